"""The score-and-select definitions of include/gpmp2mi.h ("scoring") restated in numpy on the CPU oracle:
interpolate_traj -> sphere_centers -> sdf_query, radii from the model.  Shared by tests/test_score_abi.py (oracle
only) and tests/test_gpu_score.py (the expectation of the device's scores)."""
from dataclasses import dataclass

import numpy as np

from gpmp2_amd import problems


@dataclass
class OracleField:
    """the oracle's field handle with what the comparisons need to know about the field"""
    handle: object
    dim: int
    origin: np.ndarray      # lower faces
    upper: np.ndarray       # upper faces: origin + (n - 1) * cell


def is_lie(model):
    return model.flat()["kind"] >= 2          # GPMP2MI_ROBOT_POSE2_MOBILE_BASE and up


def delta_t(setting):
    return setting.total_time / setting.total_step


def oracle_score(orc, model, ro, field, dt, inter_step, traj):
    """traj [B][N+1][2D] -> dict: the five per-row outputs plus what the comparisons need (gap: runner-up clearance
    minus the minimum per row; near_face [B]: pairs whose centre lies within 1e-9 of a field face; pairs per row)."""
    D, S = model.dof(), model.nr_body_spheres()
    t = np.ascontiguousarray(traj, dtype=np.float64).reshape(-1, np.shape(traj)[-2], 2 * D)
    B = t.shape[0]
    U = orc.interpolate_traj(D, is_lie(model), None, dt, inter_step, t)
    Md = U.shape[1]
    centers, _ = orc.sphere_centers(ro, U[:, :, :D].reshape(-1, D))
    dim = field.dim
    pts = np.ascontiguousarray(centers[:, :, :dim]).reshape(-1, dim)
    dist, _, inr = orc.sdf_query(field.handle, pts)
    dist, inr = dist.reshape(B, Md, S), inr.reshape(B, Md, S).astype(bool)
    radius = np.asarray(model.flat()["sphere_radius"], dtype=np.float64).reshape(1, 1, S)
    hinge = np.where(inr, np.where(dist > radius, 0.0, radius - dist), 0.0)
    clr = np.where(inr, dist - radius, np.inf)
    flat = clr.reshape(B, Md * S)
    arg = flat.argmin(axis=1)                 # first of equal minima: lowest state, then lowest sphere
    mn = flat[np.arange(B), arg]
    worst = np.stack([arg // S, arg % S], axis=1).astype(np.int32)
    none = ~inr.reshape(B, -1).any(axis=1)
    worst[none] = -1
    part = np.partition(flat, 1, axis=1) if Md * S > 1 else np.full((B, 2), np.inf)
    gap = part[:, 1] - part[:, 0]
    lo, hi = field.origin, field.upper
    p = pts.reshape(B, Md * S, dim)
    near = (np.abs(p - lo).min(axis=2) < 1e-9) | (np.abs(p - hi).min(axis=2) < 1e-9)
    return dict(support_cost=hinge[:, ::inter_step + 1].sum(axis=(1, 2)), dense_cost=hinge.sum(axis=(1, 2)),
                min_clearance=mn, worst=worst, out_of_range=(~inr).reshape(B, -1).sum(axis=1).astype(np.int32),
                gap=gap, near_face=near.sum(axis=1), pairs=Md * S, clearance=clr)


def oracle_sdf(orc, origin, cell, data):
    """OracleField of a field given as the problems give it (origin, cell size, [nz][ny][nx] or [ny][nx] data)"""
    data = np.asarray(data)
    n = data.shape[::-1]                      # nx, ny(, nz)
    lo = np.asarray(origin[:data.ndim], dtype=np.float64)
    return OracleField(orc.sdf(origin, cell, data), data.ndim, lo,
                       np.array([origin[a] + (n[a] - 1) * cell for a in range(data.ndim)]))


def motivation_inputs():
    """the two WAM inputs of the issue: (problem, inter_step of the dense check)"""
    return [(problems.wam_restarts(B=16, total_step=12, obs_check_inter=3, sdf="40"), 4),
            (problems.wam_restarts(B=32, total_step=20, obs_check_inter=4, sdf="40"), 5)]


def pr2_problem(B=4):
    """the dof-18 PR2 problem of scripts/pr2_time.py (N = 50, I = 2, LM), B rows"""
    import gpmp2_amd as g
    from gpmp2_amd.settings import TrajOptimizerSetting
    model = g.generateMobileArm("PR2")
    origin, cell, data = problems.small3d_sdf(40)
    origin, cell, data = list(np.array(origin) * 3), cell * 3, data * 3
    D, N = 18, 50
    st = TrajOptimizerSetting(D)
    st.set_total_step(N); st.set_total_time(10.0); st.set_obs_check_inter(2); st.set_cost_sigma(0.1); st.set_epsilon(0.4)
    st.set_conf_prior_model(1e-3); st.set_vel_prior_model(1e-3); st.set_Qc_model(np.eye(D)); st.set_max_iter(30)
    st.setLM()
    start, end = np.zeros(D), np.zeros(D)
    start[:3] = [-1.5, -1.0, 0.3]; end[:3] = [1.5, 1.2, -0.4]; end[3] = 0.2
    end[4:] = np.tile(np.linspace(0.2, 0.8, 7), 2) * np.r_[np.ones(7), -np.ones(7)]
    rng = np.random.default_rng(3)
    init = np.zeros((B, N + 1, 2 * D))
    for b in range(B):
        amp = rng.normal(0, 0.1, size=D) * (b > 0)
        for i in range(N + 1):
            init[b, i, :D] = start * (N - i) / N + end * i / N + np.sin(np.pi * i / N) * amp
        init[b, :, D:] = (end - start)[None, :] / 10.0
    z = np.zeros((B, D))
    return problems.Problem("pr2", model, origin, cell, data, st, np.repeat(start[None], B, 0), z.copy(),
                            np.repeat(end[None], B, 0), z.copy(), init)
