"""Carried object (include/gpmp2mi.h "carried object") restated in numpy on the CPU oracle: sphere centres and their
derivatives from oracle.forward_kinematics, the field from oracle.sdf_query, the hinge of the obstacle factor with the
set's own epsilon and sigma, its whitened normal-equation terms added to oracle.linearize / graph_error, a plain
Gauss-Newton loop on oracle.block_tridiag_solve, and the check of the executed trajectory on oracle.interpolate_traj.
A second, independent reference is the same robot with the carried spheres appended as body spheres (augmented): then
oracle.obstacle_factor gives the rows outright.  Shared by tests/test_carried_cpu.py (oracle only) and
tests/test_gpu_carried.py (the expectation of the device's results)."""
import copy

import numpy as np

from gpmp2_amd import robots

import moving_reference as mr
import score_reference as ref

plan_case, with_rows, PLAN_CASES = mr.plan_case, mr.with_rows, mr.PLAN_CASES


def nr_links(model):
    return model.fk_model().nr_links()


def augmented(model, link, radius, centers):
    """the same robot with the carried spheres appended as body spheres of `link`"""
    extra = [robots.BodySphere(int(link), float(r), tuple(float(x) for x in c)) for r, c in zip(radius, centers)]
    return robots.RobotModel(model.fk_model(), list(model.spheres) + extra)


# ---------------------------------------------------------------------------------------------------- the factor
def centers_and_jacobians(orc, ro, conf, link, centers):
    """conf [M][D], centers [A][3] in the frame of `link` -> c [M][A][3], dc [M][A][3][D]:
    c = T o,  d c / d q_k = R (v_k + omega_k x o),  [omega_k; v_k] column k of the link's body Jacobian"""
    poses, J = orc.forward_kinematics(ro, conf)                       # [M][L][4][4], [M][L][6][D]
    T, Jl = poses[:, link], J[:, link]
    R, t = T[:, :3, :3], T[:, :3, 3]
    o = np.asarray(centers, dtype=np.float64).reshape(-1, 3)
    c = np.einsum("mij,aj->mai", R, o) + t[:, None, :]
    om, v = Jl[:, :3, :].transpose(0, 2, 1), Jl[:, 3:, :].transpose(0, 2, 1)      # [M][D][3]
    u = v[:, None] + np.cross(om[:, None, :, :], o[None, :, None, :])               # [M][A][D][3]
    return c, np.einsum("mij,madj->maid", R, u)


def hinge_rows(orc, ro, field, conf, link, radius, centers, epsilon):
    """conf [M][D] -> err [M][A], H [M][A][D], inside [M][A], d [M][A] (field value, NaN outside)"""
    q = np.ascontiguousarray(conf, dtype=np.float64)
    M, A = q.shape[0], len(radius)
    c, dc = centers_and_jacobians(orc, ro, q, link, centers)
    dim = field.dim
    d, grad, inr = orc.sdf_query(field.handle, np.ascontiguousarray(c[:, :, :dim]).reshape(-1, dim))
    d, grad, inr = d.reshape(M, A), grad.reshape(M, A, dim), inr.reshape(M, A).astype(bool)
    te = np.asarray(radius, dtype=np.float64)[None, :] + epsilon
    with np.errstate(invalid="ignore"):
        active = inr & ~(d > te)
    err = np.where(active, te - np.where(inr, d, 0.0), 0.0)
    H = np.where(active[..., None], -np.einsum("mai,maid->mad", np.where(inr[..., None], grad, 0.0), dc[:, :, :dim]), 0.0)
    return err, H, inr, np.where(inr, d, np.nan)


def normal_terms(err, H, sigma):
    """rows err [M][A], H [M][A][D] with isotropic noise sigma -> G [M][D][D], g [M][D], e [M] (e = r^T r / 2)"""
    return mr.normal_terms(err[:, :, None], H[:, :, None, :], sigma)


def plan_terms(orc, ro, field, D, traj, cr):
    """traj [B][N+1][2D]; cr: dict(link, radius, centers, epsilon, sigma, states) -> G [B][N+1][D][D], g [B][N+1][D],
    e [B]"""
    t = np.asarray(traj, dtype=np.float64)
    B, N1 = t.shape[0], t.shape[1]
    G, gg, e = np.zeros((B, N1, D, D)), np.zeros((B, N1, D)), np.zeros(B)
    if cr is None or len(cr["radius"]) == 0:
        return G, gg, e
    first, last = cr["states"]
    idx = np.arange(first, last + 1)
    conf = np.ascontiguousarray(t[:, idx, :D]).reshape(-1, D)
    err, H, _, _ = hinge_rows(orc, ro, field, conf, cr["link"], cr["radius"], cr["centers"], cr["epsilon"])
    a, b, c = normal_terms(err, H, cr["sigma"])
    G[:, idx] = a.reshape(B, len(idx), D, D)
    gg[:, idx] = b.reshape(B, len(idx), D)
    e += c.reshape(B, len(idx)).sum(axis=1)
    return G, gg, e


_args = mr._args


def linearize(orc, ro, field, p, traj, cr):
    """oracle.linearize plus the carried terms on the configuration block of each state"""
    Hd, Ho, gr, err = orc.linearize(ro, field.handle, p.setting, *_args(p), traj)
    D = p.setting.dof
    G, gg, e = plan_terms(orc, ro, field, D, traj, cr)
    Hd[:, :, :D, :D] += G
    gr[:, :, :D] += gg
    return Hd, Ho, gr, err + e


def graph_error(orc, ro, field, p, traj, cr):
    return orc.graph_error(ro, field.handle, p.setting, *_args(p), traj) + plan_terms(orc, ro, field, p.setting.dof, traj, cr)[2]


def gauss_newton(orc, ro, field, p, cr, k, init=None):
    """the plain loop: x <- x + solve(H, -g), k times, for vector-space robots"""
    assert not ref.is_lie(p.model)
    x = np.array(p.init if init is None else init, dtype=np.float64)
    for _ in range(k):
        Hd, Ho, gr, _ = linearize(orc, ro, field, p, x, cr)
        dx, ok = orc.block_tridiag_solve(Hd, Ho, -gr)
        assert ok.all()
        x = x + dx
    return x


# ---------------------------------------------------------------------------------------------------- the check
def oracle_carried_score(orc, model, ro, field, link, radius, centers, dt, inter_step, traj):
    """traj [B][N+1][2D] -> dict: the five per-row outputs plus what the comparisons need (gap: runner-up clearance
    minus the minimum per row; clearance [B][Md][A], +inf out of range)."""
    D = model.dof()
    t = np.ascontiguousarray(traj, dtype=np.float64).reshape(-1, np.shape(traj)[-2], 2 * D)
    B, A = t.shape[0], len(radius)
    U = orc.interpolate_traj(D, ref.is_lie(model), None, dt, inter_step, t)
    Md = U.shape[1]
    if A == 0:
        return dict(carried_support_cost=np.zeros(B), carried_dense_cost=np.zeros(B),
                    min_carried_clearance=np.full(B, np.inf), worst=np.full((B, 2), -1, dtype=np.int32),
                    out_of_range=np.zeros(B, dtype=np.int32), gap=np.full(B, np.nan), clearance=np.zeros((B, Md, 0)))
    conf = np.ascontiguousarray(U[:, :, :D]).reshape(-1, D)
    _, _, inr, d = hinge_rows(orc, ro, field, conf, link, radius, centers, 0.0)
    inr, d = inr.reshape(B, Md, A), d.reshape(B, Md, A)
    r = np.asarray(radius, dtype=np.float64)[None, None, :]
    with np.errstate(invalid="ignore"):
        hinge = np.where(inr, np.where(d > r, 0.0, r - d), 0.0)
        clr = np.where(inr, d - r, np.inf)
    flat = clr.reshape(B, -1)
    arg = flat.argmin(axis=1)                 # first of equal minima: lowest state, then lowest sphere
    mn = flat[np.arange(B), arg]
    worst = np.stack([arg // A, arg % A], axis=1).astype(np.int32)
    worst[~inr.reshape(B, -1).any(axis=1)] = -1
    part = np.partition(flat, 1, axis=1) if flat.shape[1] > 1 else np.full((B, 2), np.inf)
    with np.errstate(invalid="ignore"):
        gap = part[:, 1] - part[:, 0]
    return dict(carried_support_cost=hinge[:, ::inter_step + 1].sum(axis=(1, 2)), carried_dense_cost=hinge.sum(axis=(1, 2)),
                min_carried_clearance=mn, worst=worst, out_of_range=(~inr).reshape(B, -1).sum(axis=1).astype(np.int32),
                gap=gap, clearance=clr)


close_rows = mr.close_rows


# ---------------------------------------------------------------------------------------------------------------------
# The inputs of tests/test_gpu_carried.py, built without a GPU so that tests/test_carried_cpu.py can judge them on the
# oracle.
RADIUS, SIGMA, ITERS = 0.03, 0.02, 5


def spheres(A, seed, far=True):
    """A spheres of r = 0.03 at offsets drawn in +-(0.08, 0.08, 0.2) + (0, 0, 0.2) in the link frame: a box in the hand.
    far: the last sphere (of two or more) sits 40 m out along the link's x and z axes, outside every field of the
    cases, planar ones included."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-1.0, 1.0, size=(A, 3)) * np.array([0.08, 0.08, 0.2]) + np.array([0.0, 0.0, 0.2])
    if far and A >= 2:
        c[-1] = [40.0, 0.0, 40.0]
    return np.full(A, RADIUS), np.ascontiguousarray(c)


# name -> (link, epsilon); link -1: the last link.  config5's field ends at x, y ~ 0 and its last link is outside it at
# every state, so its object rides on the base; on the PR2's inner states (N = 4) an object on the last link of the
# first arm (link 8) meets the field's obstacles, the last link of the second arm takes the second set.
FACTOR_CASES = {"arm3": (-1, 0.05), "wam": (-1, 0.05), "config5": (0, 0.05)}
PLAN_SETS = {"arm3": (-1, 0.05), "wam": (-1, 0.05), "config5": (0, 0.05), "mobile_wam": (-1, 0.05), "pr2": (8, 0.2)}
SECOND_LINK = {"arm3": 1, "wam": 3, "config5": 1, "mobile_wam": 0, "pr2": 15}
CHECK_NAMES = ("arm3", "wam", "config5", "mobile_wam")
CHECK_INTER = (0, 4)
# every (robot, inter_step) of the check, and the WAM at inter_step 6: Md = 71, two tiles of 64 checked states
CHECK_CASES = [(name, J) for name in CHECK_NAMES for J in CHECK_INTER] + [("wam", 6)]
FACTOR_AS = (1, 64, 65)


def link_of(model, link):
    return nr_links(model) - 1 if link < 0 else link


def field_of(orc, p):
    return ref.oracle_sdf(orc, p.sdf_origin, p.sdf_cell, p.sdf_data)


def middle_inactive_set(orc, ro, field, p, traj, link, epsilon, states):
    """192 spheres whose middle chunk (64..127) is inactive at every state of the range and every row: the spheres of
    the chunk sit far outside the field; the outer chunks are the ordinary box."""
    radius, centers = spheres(192, 7, far=False)
    centers[64:128] = np.array([40.0, 0.0, 40.0]) + centers[64:128]
    return radius, np.ascontiguousarray(centers)


def scenario():
    """the end-to-end scenario of the augmented-robot identity: the WAM of wam_restarts (B = 3, N = 10) with
    obs_check_inter = 0, carrying a box of 12 spheres on its last link, the factor on all states with the setting's
    epsilon and cost_sigma"""
    from gpmp2_amd import problems
    p = problems.wam_restarts(B=3, total_step=10, obs_check_inter=0, sdf="40")
    radius, centers = spheres(12, 3, far=False)
    N = p.setting.total_step
    cr = dict(link=nr_links(p.model) - 1, radius=radius, centers=centers, epsilon=p.setting.epsilon,
              sigma=p.setting.cost_sigma, states=(0, N))
    return p, cr


def augmented_problem(p, cr):
    q = copy.copy(p)
    q.model = augmented(p.model, cr["link"], cr["radius"], cr["centers"])
    return q
