"""Workspace path (include/gpmp2mi.h "workspace path") restated in numpy on the CPU oracle: the rows of
oracle.workspace_prior_factor with one target per state, their whitened normal-equation terms added to oracle.linearize /
graph_error, a plain Gauss-Newton loop on oracle.block_tridiag_solve, and the check of the executed trajectory on
oracle.interpolate_traj and oracle.forward_kinematics with the SO(3) / SE(3) maps written out here.  Shared by
tests/test_path_cpu.py (oracle only) and tests/test_gpu_path.py (the expectation of the device's results)."""
import copy

import numpy as np

import moving_reference as mr
import score_reference as ref
from moving_reference import _args, plan_case, with_rows   # noqa: F401  (the linearize cases are the moving ones)

POSITION, ORIENTATION, POSE = 0, 1, 2
EPS2 = 2.220446049250313e-16


def nrows(mode):
    return 6 if mode == POSE else 3


# ------------------------------------------------------------------------------------------- SO(3) / SE(3) maps
def skew(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def rot_exp(w):
    """Rodrigues; theta^2 <= 2.22e-16: I + [w]x"""
    w = np.asarray(w, dtype=np.float64)
    th2 = float(w @ w)
    W = skew(w)
    if th2 <= EPS2:
        return np.eye(3) + W
    th = np.sqrt(th2)
    return np.eye(3) + (np.sin(th) / th) * W + ((1.0 - np.cos(th)) / th2) * (W @ W)


def so3_k(th2):
    """k = (1 - (t / 2) cot(t / 2)) / t^2, the coefficient of [w]x^2 in the inverse Jacobians and in Pose3's Log; 1/12 at
    theta^2 <= 2.22e-16"""
    if th2 <= EPS2:
        return 1.0 / 12.0
    th = np.sqrt(th2)
    return (1.0 - 0.5 * th * np.cos(0.5 * th) / np.sin(0.5 * th)) / th2


def rot_log(R):
    """the factor's SO(3) log map (csrc/lie_log.h): theta = atan2(|v|, c) of the skew part v and c = (tr - 1) / 2; the
    axis from v while c > -1/2, from the symmetric part (largest diagonal entry) beyond, its sign from v"""
    R = np.asarray(R, dtype=np.float64)
    v = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
    c = 0.5 * (((R[0, 0] + R[1, 1]) + R[2, 2]) - 1.0)
    th = np.arctan2(s, c)
    if c > -0.5:
        return v * (th / s) if s > 0.0 else v
    i = int(np.argmax([R[0, 0], R[1, 1], R[2, 2]]))
    d = 1.0 - c
    ai = np.sqrt((R[i, i] - c) / d)
    a = np.array([(R[i, j] + R[j, i]) / (2.0 * d * ai) for j in range(3)])
    a[i] = ai
    if (a[0] * v[0] + a[1] * v[1]) + a[2] * v[2] < 0.0:
        th = -th
    return th * a


def pose_log(R, t):
    """the factor's SE(3) log map: [omega; u], u = t - w x t / 2 + k w x (w x t)"""
    w = rot_log(R)
    W = skew(w)
    Wt = W @ t
    return np.concatenate([w, t - 0.5 * Wt + so3_k(float(w @ w)) * (W @ Wt)])


def pose(R=None, t=(0.0, 0.0, 0.0)):
    T = np.eye(4)
    if R is not None:
        T[:3, :3] = R
    T[:3, 3] = t
    return T


# ---------------------------------------------------------------------------------------------------- the factor
def rows(orc, ro, mode, link, conf, des):
    """conf [M][D], des [M][4][4] (one target per evaluation) -> err [M][rows], H [M][rows][D]"""
    q = np.ascontiguousarray(conf, dtype=np.float64).reshape(-1, ro.dof)
    d = np.asarray(des, dtype=np.float64).reshape(-1, 4, 4)
    err, H = np.zeros((q.shape[0], nrows(mode))), np.zeros((q.shape[0], nrows(mode), ro.dof))
    for m in range(q.shape[0]):
        e, h = orc.workspace_prior_factor(ro, mode, link, d[m], q[m:m + 1])
        err[m], H[m] = e[0], h[0]
    return err, H


def plan_terms(orc, ro, traj, path):
    """traj [B][N+1][2D], path dict(mode, link, des [N+1][4][4], sigma [N+1]) -> G [B][N+1][D][D], g [B][N+1][D],
    e [B] (e = r^T r / 2); a state with sigma = +inf adds nothing"""
    D = ro.dof
    t = np.asarray(traj, dtype=np.float64)
    B, N1 = t.shape[0], t.shape[1]
    G, gg, e = np.zeros((B, N1, D, D)), np.zeros((B, N1, D)), np.zeros(B)
    if path is None:
        return G, gg, e
    sigma = np.broadcast_to(np.asarray(path["sigma"], dtype=np.float64), (N1,))
    for i in np.flatnonzero(np.isfinite(sigma)):
        err, H = rows(orc, ro, path["mode"], path["link"], t[:, i, :D], np.repeat(path["des"][i][None], B, 0))
        r, A = err / sigma[i], H / sigma[i]
        G[:, i] = np.einsum("bpa,bpc->bac", A, A)
        gg[:, i] = np.einsum("bpa,bp->ba", A, r)
        e += 0.5 * (r * r).sum(axis=1)
    return G, gg, e


def linearize(orc, ro, so, p, traj, path):
    """oracle.linearize plus the path terms on the configuration block of each constrained state"""
    Hd, Ho, gr, err = orc.linearize(ro, so, p.setting, *_args(p), traj)
    D = p.setting.dof
    G, gg, e = plan_terms(orc, ro, traj, path)
    Hd[:, :, :D, :D] += G
    gr[:, :, :D] += gg
    return Hd, Ho, gr, err + e


def graph_error(orc, ro, so, p, traj, path):
    return orc.graph_error(ro, so, p.setting, *_args(p), traj) + plan_terms(orc, ro, traj, path)[2]


def gauss_newton(orc, ro, so, p, path, k, init=None):
    """the plain loop: x <- x + solve(H, -g), k times, for vector-space robots"""
    assert not ref.is_lie(p.model)
    x = np.array(p.init if init is None else init, dtype=np.float64)
    for _ in range(k):
        Hd, Ho, gr, _ = linearize(orc, ro, so, p, x, path)
        dx, ok = orc.block_tridiag_solve(Hd, Ho, -gr)
        assert ok.all()
        x = x + dx
    return x


# ---------------------------------------------------------------------------------------------------- the check
def checked_targets(des, sigma, inter_step, mode):
    """des [N+1][4][4], sigma [N+1] -> (T [Md][4][4], sg [Md], checked [Md]): positions t_i + tau (t_{i+1} - t_i),
    rotations R_i Exp(tau Log(R_i^T R_{i+1})), sigma linear, tau = j / (J + 1); support states are des[i] itself"""
    des = np.asarray(des, dtype=np.float64)
    N, J = des.shape[0] - 1, inter_step
    sigma = np.broadcast_to(np.asarray(sigma, dtype=np.float64), (N + 1,))
    Md = N * (J + 1) + 1
    T, sg, chk = np.zeros((Md, 4, 4)), np.zeros(Md), np.zeros(Md, dtype=bool)
    for m in range(Md):
        i, j = divmod(m, J + 1)
        T[m], sg[m], chk[m] = des[i], sigma[i], np.isfinite(sigma[i])
        if j == 0:
            continue
        chk[m] = chk[m] and np.isfinite(sigma[i + 1])
        if not chk[m]:
            continue
        tau = float(j) / float(J + 1)
        if mode != POSITION:
            T[m, :3, :3] = des[i, :3, :3] @ rot_exp(tau * rot_log(des[i, :3, :3].T @ des[i + 1, :3, :3]))
        T[m, :3, 3] = des[i, :3, 3] + tau * (des[i + 1, :3, 3] - des[i, :3, 3])
        sg[m] = sigma[i] + tau * (sigma[i + 1] - sigma[i])
    return T, sg, chk


def oracle_path_score(orc, model, ro, mode, link, des, sigma, dt, inter_step, traj):
    """traj [B][N+1][2D] -> dict: the six per-row outputs plus pos_dev / rot_dev [B][Md] (NaN where not checked or
    invalid) and the per-row gap between the two largest deviations of each kind"""
    D = model.dof()
    t = np.ascontiguousarray(traj, dtype=np.float64).reshape(-1, np.shape(traj)[-2], 2 * D)
    B = t.shape[0]
    with np.errstate(invalid="ignore"):
        U = orc.interpolate_traj(D, ref.is_lie(model), None, dt, inter_step, t)
    Md = U.shape[1]
    T, sg, chk = checked_targets(des, sigma, inter_step, mode)
    poses, _ = orc.forward_kinematics(ro, np.ascontiguousarray(U[:, :, :D]).reshape(-1, D))
    poses = poses.reshape(B, Md, -1, 4, 4)[:, :, link]
    pos, rot = np.full((B, Md), np.nan), np.full((B, Md), np.nan)
    cost = np.zeros((B, Md))
    invalid = np.zeros(B, dtype=np.int32)
    for b in range(B):
        for m in np.flatnonzero(chk):
            P = poses[b, m]
            d = P[:3, 3] - T[m, :3, 3]
            with np.errstate(invalid="ignore"):
                Rr = T[m, :3, :3].T @ P[:3, :3]
                pd = np.sqrt(d @ d) if mode != ORIENTATION else 0.0
                w = rot_log(Rr) if mode != POSITION else np.zeros(3)
                rd = np.sqrt(w @ w)
                if mode == POSITION:
                    r2 = d @ d
                elif mode == ORIENTATION:
                    r2 = w @ w
                else:
                    xi = pose_log(Rr, T[m, :3, :3].T @ d)
                    r2 = xi @ xi
            if not (np.isfinite(pd) and np.isfinite(rd)):
                invalid[b] += 1
                continue
            pos[b, m], rot[b, m] = pd, rd
            cost[b, m] = r2 / (sg[m] * sg[m])

    def top(x, on):
        v = np.where(np.isnan(x), -np.inf, x)
        arg = v.argmax(axis=1)                       # the first of equal maxima: the lowest state
        mx = v[np.arange(B), arg]
        none = ~np.isfinite(mx) | (not on)
        srt = np.sort(v, axis=1)
        with np.errstate(invalid="ignore"):
            gap = srt[:, -1] - srt[:, -2] if Md > 1 else np.full(B, np.inf)
        return np.where(none, 0.0, mx), np.where(none, -1, arg).astype(np.int32), gap

    mp, kp, gp = top(pos, mode != ORIENTATION)
    mr_, kr, gr = top(rot, mode != POSITION)
    return dict(max_pos_dev=mp, max_rot_dev=mr_, worst=np.stack([kp, kr], axis=1), support_cost=cost[:, ::inter_step + 1].sum(axis=1),
                dense_cost=cost.sum(axis=1), invalid=invalid, pos_dev=pos, rot_dev=rot, gap_pos=gp, gap_rot=gr)


# ---------------------------------------------------------------------------------------------------------------------
# The inputs of tests/test_gpu_path.py, built without a GPU so that tests/test_path_cpu.py can judge them on the oracle.
ITERS = 5
FACTOR_CASES = {"arm3": 2, "wam": 6, "config5": 2}   # robot -> link of the factor cases (config5: a mobile kind)
PLAN_LINKS = {"arm3": 2, "wam": 6, "config5": 2, "mobile_wam": 7, "pr2": 5}


def rand_rot(rng, angle):
    u = rng.normal(size=3)
    return rot_exp(angle * u / np.linalg.norm(u))


def link_poses(orc, ro, conf, link):
    """[M][4][4]: the oracle's pose of `link` at conf [M][D]"""
    return orc.forward_kinematics(ro, np.ascontiguousarray(conf, dtype=np.float64).reshape(-1, ro.dof))[0][:, link]


def offset_targets(poses, rng, dpos=0.05, dang=0.3):
    """targets at a known offset from the poses: des = pose * (Exp(dang u), dpos v)"""
    out = np.array(poses, dtype=np.float64)
    for m in range(out.shape[0]):
        v = rng.normal(size=3)
        off = pose(rand_rot(rng, dang), dpos * v / np.linalg.norm(v))
        out[m] = out[m] @ off
    return out


def time_varying_path(orc, ro, traj_row, link, seed, sigma=0.02, gaps=()):
    """a path that differs from state to state: the link poses of one trajectory row, each moved by its own offset;
    sigma changes from state to state too; the states in `gaps` get +inf"""
    rng = np.random.default_rng(seed)
    N1 = traj_row.shape[0]
    des = offset_targets(link_poses(orc, ro, traj_row[:, :ro.dof], link), rng)
    sg = sigma * (1.0 + 0.25 * np.sin(np.arange(N1)))
    sg[list(gaps)] = np.inf
    return np.ascontiguousarray(des), sg


def piecewise_path(poses4, N):
    """[N+1][4][4]: four constant targets over the state ranges ranges4(N)"""
    des = np.zeros((N + 1, 4, 4))
    for T, (a, b) in zip(poses4, ranges4(N)):
        des[a:b + 1] = T
    return des


def ranges4(N):
    c = [0, (N + 1) // 4, (N + 1) // 2, 3 * (N + 1) // 4, N + 1]
    return [(c[k], c[k + 1] - 1) for k in range(4)]


def line_problem(B=3):
    """case (c): a WAM move of moderate size, B rows (straight line plus a sine bump), with a straight POSITION line of
    the last link between the tool positions of the start and the end configuration.  -> (problem, link)"""
    from gpmp2_amd import problems
    q = problems.wam_restarts(B=1, total_step=10, obs_check_inter=2, sdf="40")
    q.start_conf = problems.WAM_START[None]
    q.end_conf = (problems.WAM_START + np.array([0.8, 0.5, -0.4, 0.5, 0.3, 0.0, 0.0]))[None]
    return with_rows(q, B, 10, 7), 6


def line_path(orc, ro, p, link, sigma=0.001):
    from gpmp2_amd import scoring
    ends = link_poses(orc, ro, np.stack([p.start_conf[0], p.end_conf[0]]), link)
    return dict(mode=POSITION, link=link, des=scoring.line_path(ends[0], ends[1], p.setting.total_step),
                sigma=np.full(p.setting.total_step + 1, sigma))


def support_pos_dev(orc, ro, traj, link, des):
    """[B]: max over the support states of |t(q_i) - t_i|"""
    t = np.asarray(traj)
    B, N1 = t.shape[0], t.shape[1]
    P = link_poses(orc, ro, t[:, :, :ro.dof].reshape(-1, ro.dof), link).reshape(B, N1, 4, 4)
    return np.linalg.norm(P[:, :, :3, 3] - np.asarray(des)[None, :, :3, 3], axis=2).max(axis=1)


def constant_orientation_problem(opt, B=3):
    """case (a): hold the last link's orientation at that of the start configuration on all states, sigma 0.05"""
    from gpmp2_amd import problems
    p = problems.wam_restarts(B=B, total_step=10, obs_check_inter=2, sdf="40", opt=opt)
    return p, 6, 0.05


def piecewise_problem(opt, B=3):
    """case (b): four constant POSE targets of the last link over four state ranges, sigma 0.05"""
    from gpmp2_amd import problems
    p = problems.wam_restarts(B=B, total_step=10, obs_check_inter=2, sdf="40", opt=opt)
    return p, 6, 0.05


def piecewise_targets(orc, ro, p, link):
    """the link poses of the straight line at the middle of each of the four ranges"""
    N = p.setting.total_step
    mids = [(a + b) // 2 for a, b in ranges4(N)]
    return link_poses(orc, ro, p.init[0, mids, :ro.dof], link)


def native_setting(p, mode, link, poses4, sigma):
    """p's setting with the four ranges as native workspace factors of the plan / the oracle"""
    s = copy.deepcopy(p.setting)
    for T, (a, b) in zip(poses4, ranges4(s.total_step)):
        s.add_workspace_prior(mode, link, T, sigma, a, b)
    return s


def last_decision_margin(res, abs_tol=1e-5):
    """per row: |last error decrease| / abs_error_tol of a converged oracle run (how far the stop was from the threshold)"""
    out = []
    for b in range(len(res["iters"])):
        tr = res["error_trace"][b]
        tr = tr[~np.isnan(tr)]
        tr = tr[tr != 0.0] if (tr != 0.0).any() else tr
        out.append(abs(tr[-2] - tr[-1]) / abs_tol if tr.size >= 2 else np.inf)
    return np.array(out)
