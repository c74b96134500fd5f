"""Moving obstacles (include/gpmp2mi.h "moving obstacles") restated in numpy on the CPU oracle: the sphere-sphere hinge
with one sphere outside the robot on the oracle's sphere_centers (centres and Jacobians), its whitened normal-equation
terms added to oracle.linearize / graph_error, a plain Gauss-Newton loop on oracle.block_tridiag_solve, and the check of
the executed trajectory on oracle.interpolate_traj.  Shared by tests/test_moving_cpu.py (oracle only) and
tests/test_gpu_moving.py (the expectation of the device's results)."""
import copy

import numpy as np

import gpmp2_amd as g
from gpmp2_amd import problems
from gpmp2_amd.settings import TrajOptimizerSetting

import score_reference as ref


def robot_radius(model):
    return np.asarray(model.flat()["sphere_radius"], dtype=np.float64)


def total_eps(model, radius, epsilon):
    """[S][K]: (r_s + radius_k) + epsilon, in that order"""
    return (robot_radius(model)[:, None] + np.asarray(radius, dtype=np.float64)[None, :]) + epsilon


# ---------------------------------------------------------------------------------------------------- the factor
def hinge_rows(orc, model, ro, conf, radius, centers, epsilon):
    """conf [M][D], radius [K], centers [M][K][3] -> err [M][S][K], H [M][S][K][D], dist [M][S][K]"""
    D = model.dof()
    q = np.ascontiguousarray(conf, dtype=np.float64).reshape(-1, D)
    c, J = orc.sphere_centers(ro, q)                                  # [M][S][3], [M][S][3][D]
    o = np.asarray(centers, dtype=np.float64).reshape(q.shape[0], -1, 3)
    d = c[:, :, None, :] - o[:, None, :, :]                           # [M][S][K][3]
    dist = np.sqrt((d * d).sum(axis=3))
    te = total_eps(model, radius, epsilon)[None]
    active = ~(dist > te)
    err = np.where(active, te - dist, 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        n = np.where((active & (dist != 0.0))[..., None], d / dist[..., None], 0.0)
    H = -np.einsum("mskq,msqd->mskd", n, J)
    return err, H, dist


def normal_terms(err, H, sigma):
    """rows err [M][S][K], H [M][S][K][D] with isotropic noise sigma -> G [M][D][D], g [M][D], e [M] (e = r^T r / 2)"""
    M, D = err.shape[0], H.shape[-1]
    r = err.reshape(M, -1) / sigma
    A = H.reshape(M, -1, D) / sigma
    return np.einsum("mpa,mpb->mab", A, A), np.einsum("mpa,mp->ma", A, r), 0.5 * (r * r).sum(axis=1)


def plan_terms(orc, model, ro, traj, radius, centers, epsilon, sigma, states):
    """traj [B][N+1][2D], centers [K][N+1][3], states (first, last) -> G [B][N+1][D][D], g [B][N+1][D], e [B]"""
    D = model.dof()
    t = np.asarray(traj, dtype=np.float64)
    B, N1 = t.shape[0], t.shape[1]
    G, gg, e = np.zeros((B, N1, D, D)), np.zeros((B, N1, D)), np.zeros(B)
    K = len(radius)
    if K == 0:
        return G, gg, e
    first, last = states
    idx = np.arange(first, last + 1)
    conf = t[:, idx, :D].reshape(-1, D)
    cen = np.broadcast_to(np.asarray(centers, dtype=np.float64)[:, idx, :].transpose(1, 0, 2)[None], (B, len(idx), K, 3))
    err, H, _ = hinge_rows(orc, model, ro, conf, radius, cen.reshape(-1, K, 3), epsilon)
    a, b, c = normal_terms(err, H, sigma)
    G[:, idx] = a.reshape(B, len(idx), D, D)
    gg[:, idx] = b.reshape(B, len(idx), D)
    e += c.reshape(B, len(idx)).sum(axis=1)
    return G, gg, e


def _args(p):
    return p.start_conf, p.start_vel, p.end_conf, p.end_vel


def linearize(orc, ro, so, p, traj, mv):
    """oracle.linearize plus the moving terms on the configuration block of each state; mv: dict(radius, centers,
    epsilon, sigma, states) or None"""
    Hd, Ho, gr, err = orc.linearize(ro, so, p.setting, *_args(p), traj)
    if mv is not None and len(mv["radius"]):
        D = p.setting.dof
        G, gg, e = plan_terms(orc, p.model, ro, traj, mv["radius"], mv["centers"], mv["epsilon"], mv["sigma"], mv["states"])
        Hd[:, :, :D, :D] += G
        gr[:, :, :D] += gg
        err = err + e
    return Hd, Ho, gr, err


def graph_error(orc, ro, so, p, traj, mv):
    err = orc.graph_error(ro, so, p.setting, *_args(p), traj)
    if mv is not None and len(mv["radius"]):
        err = err + plan_terms(orc, p.model, ro, traj, mv["radius"], mv["centers"], mv["epsilon"], mv["sigma"],
                               mv["states"])[2]
    return err


def gauss_newton(orc, ro, so, p, mv, k, init=None):
    """the plain loop: x <- x + solve(H, -g), k times, for vector-space robots"""
    assert not ref.is_lie(p.model)
    x = np.array(p.init if init is None else init, dtype=np.float64)
    for _ in range(k):
        Hd, Ho, gr, _ = linearize(orc, ro, so, p, x, mv)
        dx, ok = orc.block_tridiag_solve(Hd, Ho, -gr)
        assert ok.all()
        x = x + dx
    return x


# ---------------------------------------------------------------------------------------------------- the check
def sphere_positions(centers, inter_step):
    """centers [K][N+1][3] -> [K][Md][3]: o_i + tau (o_{i+1} - o_i), tau = j / (J + 1); support states are o_i itself"""
    c = np.asarray(centers, dtype=np.float64)
    K, N = c.shape[0], c.shape[1] - 1
    J = inter_step
    out = np.zeros((K, N * (J + 1) + 1, 3))
    for i in range(N):
        for j in range(J + 1):
            tau = float(j) / float(J + 1)
            out[:, i * (J + 1) + j] = c[:, i] if j == 0 else c[:, i] + tau * (c[:, i + 1] - c[:, i])
    out[:, -1] = c[:, N]
    return out


def oracle_moving_score(orc, model, ro, radius, centers, epsilon, dt, inter_step, traj):
    """traj [B][N+1][2D] -> dict: the five per-row outputs plus what the comparisons need (gap: runner-up clearance
    minus the minimum per row; clearance [B][Md][S][K], +inf where invalid)."""
    D, S = model.dof(), model.nr_body_spheres()
    t = np.ascontiguousarray(traj, dtype=np.float64).reshape(-1, np.shape(traj)[-2], 2 * D)
    B, K = t.shape[0], len(radius)
    with np.errstate(invalid="ignore"):
        U = orc.interpolate_traj(D, ref.is_lie(model), None, dt, inter_step, t)
    Md = U.shape[1]
    if K == 0:
        return dict(moving_support_cost=np.zeros(B), moving_dense_cost=np.zeros(B), min_moving_clearance=np.full(B, np.inf),
                    worst=np.full((B, 3), -1, dtype=np.int32), invalid=np.zeros(B, dtype=np.int32), gap=np.full(B, np.nan),
                    clearance=np.zeros((B, Md, S, 0)))
    c, _ = orc.sphere_centers(ro, np.ascontiguousarray(U[:, :, :D]).reshape(-1, D))
    c = c.reshape(B, Md, S, 3)
    o = sphere_positions(centers, inter_step).transpose(1, 0, 2)      # [Md][K][3]
    d = c[:, :, :, None, :] - o[None, :, None, :, :]
    with np.errstate(invalid="ignore", over="ignore"):
        dist = np.sqrt((d * d).sum(axis=4))                           # [B][Md][S][K]
    te = total_eps(model, radius, epsilon)[None, None]
    valid = np.isfinite(dist)
    with np.errstate(invalid="ignore"):
        hinge = np.where(valid, np.where(dist > te, 0.0, te - dist), 0.0)
        clr = np.where(valid, dist - te, np.inf)
    flat = clr.reshape(B, -1)
    arg = flat.argmin(axis=1)                 # first of equal minima: lowest state, then sphere, then moving sphere
    mn = flat[np.arange(B), arg]
    worst = np.stack([arg // (S * K), (arg // K) % S, arg % K], axis=1).astype(np.int32)
    worst[~valid.reshape(B, -1).any(axis=1)] = -1
    part = np.partition(flat, 1, axis=1) if flat.shape[1] > 1 else np.full((B, 2), np.inf)
    with np.errstate(invalid="ignore"):
        gap = part[:, 1] - part[:, 0]
    return dict(moving_support_cost=hinge[:, ::inter_step + 1].sum(axis=(1, 2, 3)), moving_dense_cost=hinge.sum(axis=(1, 2, 3)),
                min_moving_clearance=mn, worst=worst, invalid=(~valid).reshape(B, -1).sum(axis=1).astype(np.int32),
                gap=gap, clearance=clr)


def close_rows(exp):
    """number of rows whose runner-up is within 1e-6 of the minimum: the rows a `worst` comparison may excuse"""
    with np.errstate(invalid="ignore"):
        return int((exp["gap"] <= 1e-6).sum())


# ---------------------------------------------------------------------------------------------------------------------
# The inputs of tests/test_gpu_moving.py, built without a GPU so that tests/test_moving_cpu.py can judge them on the
# oracle.
EPSILON, SIGMA, ITERS = 0.2, 0.01, 5


def scenario():
    """the end-to-end scenario: (problem, mv).  Two spheres cross the path of the WAM's outer spheres around mid-way."""
    p = problems.wam_restarts(B=3, total_step=10, obs_check_inter=2, sdf="40")
    N, S, K = p.setting.total_step, p.model.nr_body_spheres(), 2
    rng = np.random.default_rng(2)
    sk = rng.integers(S // 2, S, K)
    radius = rng.uniform(0.03, 0.08, K)
    u = rng.normal(size=(K, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    tm = rng.uniform(-0.4, 0.4, K)
    return p, dict(sk=sk, radius=radius, u=u, tm=tm, epsilon=EPSILON, sigma=SIGMA, states=(0, N))


def scenario_centers(orc, ro, p, mv):
    """centers[k][i] = c_sk(init[0], state N // 2) + u_k 1.2 (t_i - tm_k), t = linspace(-1, 1, N + 1)"""
    N, D = p.setting.total_step, p.setting.dof
    c, _ = orc.sphere_centers(ro, p.init[0, N // 2, :D][None])
    t = np.linspace(-1.0, 1.0, N + 1)
    return np.ascontiguousarray(c[0, mv["sk"]][:, None, :] + mv["u"][:, None, :] * 1.2 * (t[None, :, None] - mv["tm"][:, None, None]))


def support_clearance(orc, model, ro, traj, radius, centers, epsilon):
    """[B]: min over support states, spheres and moving spheres of dist - total_eps"""
    D = model.dof()
    t = np.asarray(traj)
    B, N1, K = t.shape[0], t.shape[1], len(radius)
    cen = np.broadcast_to(np.asarray(centers).transpose(1, 0, 2)[None], (B, N1, K, 3)).reshape(-1, K, 3)
    _, _, dist = hinge_rows(orc, model, ro, t[:, :, :D].reshape(-1, D), radius, cen, epsilon)
    return (dist - total_eps(model, radius, epsilon)[None]).reshape(B, -1).min(axis=1)


def with_rows(p, B, N, seed, amp=0.1):
    """p's robot, field and setting at B rows of N steps: straight lines with a sine bump (row 0: none)"""
    q = copy.deepcopy(p)
    s = q.setting
    s.set_total_step(N)
    D = s.dof
    start, end = np.asarray(p.start_conf[0]), np.asarray(p.end_conf[0])
    rng = np.random.default_rng(seed)
    i = np.arange(N + 1)[:, None] / N
    init = np.zeros((B, N + 1, 2 * D))
    for b in range(B):
        a = rng.normal(0.0, amp, size=D) * (b > 0)
        init[b, :, :D] = start + (end - start) * i + np.sin(np.pi * i) * a
        init[b, :, D:] = (end - start) / s.total_time
    z = np.zeros((B, D))
    q.start_conf, q.end_conf = np.repeat(start[None], B, 0), np.repeat(end[None], B, 0)
    q.start_vel, q.end_vel, q.init = z, z.copy(), init
    return q


def mobile_wam_problem(B, N):
    """SE(2) base + WAM (dof 10): a plan with blocks wider than one tile"""
    wam = g.generateArm("WAMArm")
    a7 = wam.fk_model()
    mob = g.Pose2MobileArm(g.Arm(7, a7.a, a7.alpha, a7.d), g.pose3(t=(0.0, 0.0, 0.3)))
    model = g.ArmModel(mob, [g.BodySphere(0, 0.3, (0, 0, 0.15))] + [g.BodySphere(s.link_id + 1, s.radius, s.center) for s in wam.spheres])
    origin, cell, data = problems.small3d_sdf(40)
    origin, cell, data = list(np.array(origin) * 3), cell * 3, data * 3
    D = 10
    st = TrajOptimizerSetting(D)
    st.set_total_step(N); st.set_total_time(10.0); st.set_obs_check_inter(2); st.set_cost_sigma(0.05); st.set_epsilon(0.3)
    st.set_conf_prior_model(1e-3); st.set_vel_prior_model(1e-3); st.set_Qc_model(np.eye(D)); st.set_max_iter(50)
    st.setLM()
    start = np.concatenate([[-2.0, -1.5, 0.0], problems.WAM_START])[None]
    end = np.concatenate([[2.0, 1.5, 0.5], problems.WAM_END])[None]
    z = np.zeros((1, D))
    return with_rows(problems.Problem("mobile_wam", model, origin, cell, data, st, start, z, end, z.copy(), None), B, N, 5, 0.3)


def plan_case(name):
    """the B = 3 problems of the linearize cases: (problem, perturbed trajectory)"""
    if name == "arm3":
        p = with_rows(problems.arm3_planner(), 3, 10, 11)
    elif name == "wam":
        p = problems.wam_restarts(B=3, total_step=10, obs_check_inter=2, sdf="40", opt="LM")
    elif name == "config5":
        p = with_rows(problems.mobile_arm_config5(), 3, 10, 12)
    elif name == "mobile_wam":
        p = mobile_wam_problem(3, 10)
    elif name == "pr2":
        p = with_rows(ref.pr2_problem(1), 3, 4, 13)
    else:
        raise KeyError(name)
    rng = np.random.default_rng(len(name))
    return p, p.init + 0.05 * rng.normal(size=p.init.shape)


PLAN_CASES = ("arm3", "wam", "config5", "mobile_wam", "pr2")


def spheres_near(orc, model, ro, traj, K, seed, epsilon):
    """K moving spheres for a trajectory batch: sphere k follows body sphere s_k of row 0 at an offset of known length
    around total_eps (shorter for even k, longer for odd k), so that both hinge branches occur.  -> radius [K],
    centers [K][N+1][3]"""
    D, S = model.dof(), model.nr_body_spheres()
    t = np.asarray(traj)
    N1 = t.shape[1]
    rng = np.random.default_rng(seed)
    sk = rng.integers(0, S, K)
    radius = rng.uniform(0.03, 0.08, K)
    u = rng.normal(size=(K, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    c, _ = orc.sphere_centers(ro, np.ascontiguousarray(t[0, :, :D]))
    te = total_eps(model, radius, epsilon)[sk, np.arange(K)]
    length = te * np.where(np.arange(K) % 2 == 0, 0.6, 1.0 + 0.5 * np.arange(K))
    wob = 1.0 + 0.1 * np.sin(np.arange(N1))            # the distance changes from state to state
    return radius, np.ascontiguousarray(c[:, sk].transpose(1, 0, 2) + u[:, None, :] * length[:, None, None] * wob[None, :, None])


# the check: (robot, (N, J), K) at the tile edges Md = 11, 64, 65
CHECK_SIZES = ((10, 0), (21, 2), (16, 3))
CHECK_KS = (0, 1, 5)
CHECK_DT = 0.25


def check_models():
    import self_reference as sr
    m = sr.models()
    return dict(arm3=m["arm3s"], wam=m["wam"], config5=m["config5"])


def check_traj(name, N):
    import self_reference as sr
    return sr.case_traj({"arm3": "arm3s"}.get(name, name), N)


CHECK_CASES = [(name, size, K) for name in ("arm3", "wam", "config5") for size in CHECK_SIZES for K in CHECK_KS
               if name == "wam" or (size, K) in (((21, 2), 5), ((16, 3), 1))]


def check_id(c):
    return f"{c[0]}-N{c[1][0]}J{c[1][1]}-K{c[2]}"
