"""Pins the yardstick of tests/posterior_reference.py on the CPU oracle's `linearize` (no GPU needed), and checks the
posterior entry points of the C ABI as far as they go without a device.

On the WAM (sdf "40", B = 2, N = 2, 5, 16) and mobile_arm_config5, against the long-double recursion, measured here:
the float64 recursion e = 2.4e-15 .. 1.7e-13 (WAM), 6.6e-12 (config 5); np.linalg.inv of the dense matrix 2.8e-15 ..
1.8e-13 and 2.6e-12; cond(H) 1.3e7 .. 1.9e9; the float64 sampling solve 2.5e-15 .. 4.7e-12.  A relative slip of 1e-6 in
one entry of G_0 or G_2 (WAM, N = 5) gives e = 5.1e-9 and 6.6e-8, of 1e-8 5.1e-11 and 6.6e-10.  CAP = 1e-9, the ceiling of
the GPU bound (tests/test_gpu_posterior.py), therefore lets every float64 yardstick pass and stops the 1e-6 slip; this
file asserts both."""
import ctypes

import numpy as np
import pytest

import posterior_reference as ref
from gpmp2_amd import problems

CAP = 1e-9


def _args(p):
    return p.start_conf, p.start_vel, p.end_conf, p.end_vel


def _wam(N, inter):
    return problems.wam_restarts(B=2, total_step=N, obs_check_inter=inter, opt="GN", sdf="40")


CASES = [pytest.param(lambda: _wam(2, 1), id="wam-N2-I1"), pytest.param(lambda: _wam(5, 2), id="wam-N5-I2"),
         pytest.param(lambda: _wam(16, 2), id="wam-N16-I2"), pytest.param(problems.mobile_arm_config5, id="config5")]


def _linearize(oracle, p):
    ro, so = oracle.robot(p.model), oracle.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)
    Hd, Ho, _, _ = oracle.linearize(ro, so, p.setting, *_args(p), p.init)
    return Hd, Ho


@pytest.mark.parametrize("make", CASES)
def test_float64_yardsticks_stay_below_cap(oracle, make):
    p = make()
    Hd, Ho = _linearize(oracle, p)
    for b in range(Hd.shape[0]):
        tr = ref.truth(Hd[b], Ho[b])
        e_rec = ref.cov_error(*ref.marginals(Hd[b], Ho[b]), *tr)
        e_inv = ref.cov_error(*ref.dense_inv_band(Hd[b], Ho[b]), *tr)
        print(f"trajectory {b}: e recursion {e_rec:.2e}, dense inv {e_inv:.2e}, cond(H) "
              f"{np.linalg.cond(ref.dense(Hd[b], Ho[b])):.2e}, variances {float(ref.sigma_of(tr[0]).min()) ** 2:.1e} .. "
              f"{float(ref.sigma_of(tr[0]).max()) ** 2:.1e}")
        assert max(e_rec, e_inv) < CAP
        assert ref.cpu_yardstick(Hd[b], Ho[b], tr) == max(e_rec, e_inv)
        # the truth is a truth: Sigma H = I on the block rows the band covers, in long double
        Sd, So = tr
        Hl, Hol = Hd[b].astype(ref.LD), Ho[b].astype(ref.LD)
        n, nb = Hd.shape[-1], Hd.shape[1]
        for i in (0, nb // 2, nb - 1):
            r = Sd[i] @ Hl[i] - np.eye(n, dtype=ref.LD)
            if i > 0:
                r += So[i - 1] @ Hol[i - 1].T        # Sigma_{i,i-1} H_{i-1,i}
            if i + 1 < nb:
                r += So[i].T @ Hol[i]                # Sigma_{i,i+1} H_{i+1,i}
            assert float(np.abs(r).max()) < 1e-9, i   # cond * eps_longdouble
        assert np.array_equal(Sd, np.swapaxes(Sd, 1, 2))


def test_injected_slip_exceeds_cap(oracle):
    """the 1e-6 slip in one entry of G_0 or G_2 must not pass CAP; the 1e-8 one shows the measure scales with it"""
    Hd, Ho = _linearize(oracle, _wam(5, 2))
    Hd, Ho = Hd[0], Ho[0]
    tr = ref.truth(Hd, Ho)
    for i in (0, 2):
        e6 = ref.cov_error(*ref.marginals(Hd, Ho, slip=(i, 1, 2, 1e-6)), *tr)
        e8 = ref.cov_error(*ref.marginals(Hd, Ho, slip=(i, 1, 2, 1e-8)), *tr)
        print(f"slip in G_{i}: e = {e6:.2e} (1e-6), {e8:.2e} (1e-8)")
        assert e6 > CAP
        assert 10 * e8 < e6


@pytest.mark.parametrize("make", CASES)
def test_sampling_solve(oracle, make):
    """delta = L^-T z: float64 against long double on the sigma scale, and delta^T H delta = z^T z (cov(delta) = H^-1)"""
    p = make()
    Hd, Ho = _linearize(oracle, p)
    Hd, Ho = Hd[0], Ho[0]
    nb, n = Hd.shape[0], Hd.shape[1]
    z = np.random.default_rng(11).normal(size=(3, nb, n))
    d = ref.truth_sample(Hd, Ho, z)
    e = ref.sample_error(ref.sample(Hd, Ho, z), d, ref.truth(Hd, Ho)[0])
    print(f"float64 sampling solve against long double: {e:.2e}")
    assert e < CAP
    H = ref.dense(Hd.astype(ref.LD), Ho.astype(ref.LD))
    for k in range(z.shape[0]):
        v = d[k].reshape(-1)
        assert float(abs(v @ H @ v - (z[k] ** 2).sum())) < 1e-9 * (z[k] ** 2).sum()


def test_measure_sees_the_tight_states():
    """two uncoupled scalar blocks, variances 1e-8 and 1: an absolute error of 1e-12 in the tight one is e = 1e-4"""
    Sd = np.array([[[1e-8]], [[1.0]]])
    So = np.zeros((1, 1, 1))
    bad = Sd.copy()
    bad[0] += 1e-12
    assert ref.cov_error(bad, So, Sd, So) == pytest.approx(1e-4, rel=1e-6)
    bad = Sd.copy()
    bad[1] += 1e-12
    assert ref.cov_error(bad, So, Sd, So) == pytest.approx(1e-12, rel=1e-3)
    assert ref.cov_error(None, So + 1e-6, Sd, So) == pytest.approx(1e-6 / 1e-4, rel=1e-9)


# ---------------------------------------------------------------------------------------------- the C ABI, no device
def _lib():
    from gpmp2_amd import engine
    return engine.Engine()


def test_posterior_entry_points_have_the_declared_signatures():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pub = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "gpmp2mi.h")).read(), flags=re.S)
    pub = re.sub(r"\s+", " ", pub)
    for decl in (
        "int gpmp2mi_block_tridiag_marginals(int B, int nblk, int n, const double* Hdiag, const double* Hoff, "
        "double* Sdiag, double* Soff, int* ok);",
        "int gpmp2mi_block_tridiag_sample(int B, int nblk, int n, int K, const double* Hdiag, const double* Hoff, "
        "const double* z, double* delta, int* ok);",
        "int gpmp2mi_plan_marginals(gpmp2mi_plan* p, const double* traj, double* Sdiag, double* Soff, int* ok);",
        "int gpmp2mi_plan_marginals_dev(gpmp2mi_plan* p, double* Sdiag, double* Soff, int* ok, void* stream);",
        "int gpmp2mi_plan_sample_posterior(gpmp2mi_plan* p, int K, const double* z, double* delta, int* ok);",
        "int gpmp2mi_plan_sample_posterior_dev(gpmp2mi_plan* p, int K, const double* z, double* delta, int* ok, "
        "void* stream);",
    ):
        assert decl in pub, decl
    lib = _lib().lib
    for name in ("gpmp2mi_block_tridiag_marginals", "gpmp2mi_block_tridiag_sample", "gpmp2mi_plan_marginals",
                 "gpmp2mi_plan_marginals_dev", "gpmp2mi_plan_sample_posterior", "gpmp2mi_plan_sample_posterior_dev"):
        assert getattr(lib, name).argtypes is not None, name


def test_bad_arguments_are_refused_before_any_device_work():
    from gpmp2_amd import engine
    eng = _lib()
    lib = eng.lib
    H = np.tile(np.eye(2), (1, 3, 1, 1))
    O = np.zeros((1, 2, 2, 2))
    z = np.zeros((1, 1, 3, 2))
    d, i = engine.dptr, engine.iptr
    ok = np.zeros(1, dtype=np.int32)
    marg, samp = lib.gpmp2mi_block_tridiag_marginals, lib.gpmp2mi_block_tridiag_sample
    # NULL systems, sizes
    assert marg(1, 3, 2, None, d(O), d(H), None, i(ok)) == 1 and b"null" in lib.gpmp2mi_last_error()
    assert marg(1, 3, 2, d(H), None, d(H), None, i(ok)) == 1
    assert marg(1, 0, 2, d(H), d(O), d(H), None, i(ok)) == 1
    assert marg(-1, 3, 2, d(H), d(O), d(H), None, i(ok)) == 1
    assert samp(1, 3, 2, 1, None, d(O), d(z), d(z), None) == 1
    assert samp(1, 3, 2, 1, d(H), d(O), None, d(z), None) == 1 and b"z" in lib.gpmp2mi_last_error()
    assert samp(1, 3, 2, 1, d(H), d(O), d(z), None, None) == 1
    assert samp(1, 3, 2, 0, d(H), d(O), d(z), d(z), None) == 1 and b"K" in lib.gpmp2mi_last_error()
    # one tile per block
    H16 = np.tile(np.eye(16), (1, 2, 1, 1))
    O16 = np.zeros((1, 1, 16, 16))
    z16 = np.zeros((1, 1, 2, 16))
    assert marg(1, 2, 16, d(H16), d(O16), d(H16.copy()), None, None) == 4 and b"1..15" in lib.gpmp2mi_last_error()
    assert samp(1, 2, 16, 1, d(H16), d(O16), d(z16), d(z16.copy()), None) == 4
    # NULL plans
    assert lib.gpmp2mi_plan_marginals(None, None, d(H), None, None) == 1 and b"null plan" in lib.gpmp2mi_last_error()
    assert lib.gpmp2mi_plan_marginals_dev(None, None, None, None, None) == 1
    assert lib.gpmp2mi_plan_sample_posterior(None, 1, d(z), d(z), None) == 1
    assert lib.gpmp2mi_plan_sample_posterior_dev(None, 1, ctypes.c_void_p(8), ctypes.c_void_p(8), None, None) == 1
    # B = 0 does nothing, device or not
    assert marg(0, 3, 2, d(H), d(O), None, None, None) == 0


def test_without_a_gpu_the_calls_say_so():
    """no quiet fall-back: GPMP2MI_ERR_NO_DEVICE without a device (with one, the same calls succeed)"""
    from gpmp2_amd import engine
    eng = _lib()
    lib = eng.lib
    want = 0 if eng.device_count() > 0 else 2
    H = np.tile(2.0 * np.eye(2), (1, 3, 1, 1))
    O = np.zeros((1, 2, 2, 2))
    S, z = np.zeros_like(H), np.ones((1, 1, 3, 2))
    dl = np.zeros_like(z)
    ok = np.zeros(1, dtype=np.int32)
    d, i = engine.dptr, engine.iptr
    assert lib.gpmp2mi_block_tridiag_marginals(1, 3, 2, d(H), d(O), d(S), None, i(ok)) == want
    assert lib.gpmp2mi_block_tridiag_sample(1, 3, 2, 1, d(H), d(O), d(z), d(dl), i(ok)) == want
    if want == 0:
        assert np.abs(S - np.tile(0.5 * np.eye(2), (1, 3, 1, 1))).max() <= 1e-15 and ok[0] == 1     # (1 / sqrt 2)^2
        assert np.abs(dl - np.sqrt(0.5)).max() <= 1e-15


def test_wrapper_rejects_bad_shapes_before_the_library():
    from gpmp2_amd import engine

    class NoLib:
        def __getattr__(self, name):
            raise AssertionError(f"reached the library: {name}")

    class Eng:
        lib = NoLib()

    pl = engine.Plan.__new__(engine.Plan)
    pl.eng, pl.B, pl.D, pl.N, pl.h = Eng(), 2, 3, 4, None
    with pytest.raises(ValueError, match="z: expected"):
        pl.sample_posterior(np.zeros((2, 1, 4, 6)))
    with pytest.raises(ValueError, match="K >= 1"):
        pl.sample_posterior(np.zeros((2, 0, 5, 6)))
    with pytest.raises(ValueError, match="K must be"):
        pl.sample_posterior_dev(0, 8, 8)
    with pytest.raises(ValueError, match="required"):
        pl.sample_posterior_dev(1, None, 8)
