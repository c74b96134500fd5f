"""The rule of include/gpmp2mi.h "goal configurations" restated in numpy float64 over the CPU oracle's
workspace_prior_factor / forward_kinematics (tests/oracle.py, imported as is): the damped least-squares iteration, the
seeded draw (tests/rng_reference.py), the clearance of an answer (the oracle's sphere_centers + sdf_query) and the goal
rule (scoring.group_rule).  All rows of one pose advance together; a row leaves at its own count.

Also the cases that tests/test_ik_cpu.py pins, tests/test_gpu_ik.py compares the device with and scripts/ik_error.py
measures, and the reference's own sensitivity to its seeds (d_self)."""
from dataclasses import dataclass, field, replace

import numpy as np

import gpmp2_amd as g
import rng_reference as R
from gpmp2_amd import scoring

POSITION, ORIENTATION, POSE = 0, 1, 2
CONVERGED, MAX_ITER_REACHED, INVALID = 0, 1, 2
RNG_IK = 4

WAM_DOWN = np.array([-2.6, -2.0, -2.8, -0.9, -4.76, -1.6, -3.0])
WAM_UP = np.array([2.6, 2.0, 2.8, 3.1, 1.24, 1.6, 3.0])


@dataclass
class Opts:
    """gpmp2mi_ik_opts with the defaults of gpmp2mi_ik_opts_default; clamp = False is the deliberate slip of
    tests/test_ik_cpu.py, never the rule"""
    mode: int = POSE
    link: int = 0
    pos_tol: float = 1e-6
    rot_tol: float = 1e-6
    rot_weight: float = 1.0
    max_iter: int = 100
    lambda_initial: float = 1e-2
    lambda_factor: float = 4.0
    lambda_lower: float = 1e-9
    lambda_upper: float = 1e6
    down: np.ndarray = None
    up: np.ndarray = None
    clamp: bool = True


def _clamp(o, x):
    if o.down is None or not o.clamp:
        return x
    return np.minimum(np.maximum(x, o.down), o.up)


def _norm3(v):
    return np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])


def row_scale(o):
    """the factor of every row of e / H: rot_weight on the omega rows"""
    if o.mode == POSE:
        return np.array([o.rot_weight] * 3 + [1.0] * 3)
    return np.full(3, o.rot_weight if o.mode == ORIENTATION else 1.0)


def converged(o, e):
    if o.mode == POSE:
        return (_norm3(e[:, :3]) <= o.rot_tol) & (_norm3(e[:, 3:]) <= o.pos_tol)
    return _norm3(e) <= (o.rot_tol if o.mode == ORIENTATION else o.pos_tol)


def residual(o, e):
    z = np.zeros(e.shape[0])
    if o.mode == POSE:
        return np.stack([_norm3(e[:, :3]), _norm3(e[:, 3:])], axis=1)
    return np.stack([_norm3(e), z] if o.mode == ORIENTATION else [z, _norm3(e)], axis=1)


def cost(o, e):
    x = e * row_scale(o)
    c = np.zeros(e.shape[0])
    for r in range(e.shape[1]):   # ascending r
        c = c + x[:, r] * x[:, r]
    return c


def _solve(A, b):
    """Cholesky solve of the stacked SPD systems A [P][r][r] y = b [P][r], by the loops of the rule -> (y, bad): bad
    where a pivot is not positive (NaN included)"""
    P, r = b.shape
    L = np.zeros_like(A)
    bad = np.zeros(P, dtype=bool)
    with np.errstate(invalid="ignore", divide="ignore"):
        for j in range(r):
            d = A[:, j, j].copy()
            for k in range(j):
                d -= L[:, j, k] * L[:, j, k]
            bad |= ~(d > 0.0)
            L[:, j, j] = np.sqrt(d)
            for i in range(j + 1, r):
                s = A[:, i, j].copy()
                for k in range(j):
                    s -= L[:, i, k] * L[:, j, k]
                L[:, i, j] = s / L[:, j, j]
        y = np.zeros_like(b)
        for i in range(r):
            s = b[:, i].copy()
            for k in range(i):
                s -= L[:, i, k] * y[:, k]
            y[:, i] = s / L[:, i, i]
        for i in range(r - 1, -1, -1):
            s = y[:, i].copy()
            for k in range(i + 1, r):
                s -= L[:, k, i] * y[:, k]
            y[:, i] = s / L[:, i, i]
    return y, bad


def solve(orc, ro, o, des_pose, seeds):
    """one pose: des_pose [4][4], seeds [M][D] -> dict(conf [M][D], residual [M][2], iters [M], status [M])"""
    seeds = np.ascontiguousarray(seeds, dtype=np.float64)
    M, D = seeds.shape
    sc = row_scale(o)

    def factor(q):
        with np.errstate(invalid="ignore"):
            return orc.workspace_prior_factor(ro, o.mode, o.link, des_pose, q)

    q = _clamp(replace(o, clamp=True), seeds)       # the seed is always clamped: the slip is in the steps
    e, H = factor(q)
    c = cost(o, e)
    it = np.zeros(M, dtype=np.int32)
    status = np.full(M, MAX_ITER_REACHED, dtype=np.int32)
    invalid = ~(np.isfinite(seeds).all(axis=1) & np.isfinite(e).all(axis=1))
    status[invalid] = INVALID
    conv = converged(o, e) & ~invalid
    status[conv] = CONVERGED
    active = ~invalid & ~conv
    lam = np.full(M, o.lambda_initial)
    while active.any():
        ix = np.flatnonzero(active)
        Hh, eh = H[ix] * sc[None, :, None], e[ix] * sc[None, :]
        A = np.einsum("pik,pjk->pij", Hh, Hh) + lam[ix, None, None] * np.eye(eh.shape[1])[None]
        y, bad = _solve(A, eh)
        dq = -np.einsum("prk,pr->pk", Hh, y)
        qn = np.where(bad[:, None], q[ix], _clamp(o, q[ix] + dq))
        en, Hn = factor(qn)
        cn = cost(o, en)
        it[ix] += 1
        with np.errstate(invalid="ignore"):
            acc = ~bad & (cn < c[ix])
        a = ix[acc]
        q[a], e[a], H[a], c[a] = qn[acc], en[acc], Hn[acc], cn[acc]
        lam[a] = np.maximum(lam[a] / o.lambda_factor, o.lambda_lower)
        rej = ix[~acc]
        lam[rej] = np.minimum(lam[rej] * o.lambda_factor, o.lambda_upper)
        done = a[converged(o, e[a])]
        status[done] = CONVERGED
        active[done] = False
        active[it >= o.max_iter] = False
    return dict(conf=q, residual=residual(o, e), iters=it, status=status)


def solve_all(orc, ro, o, des_poses, seeds):
    """des_poses [G][4][4], seeds [G][M][D] -> the outputs of gpmp2mi_ik_solve, stacked over the poses"""
    rows = [solve(orc, ro, o, des_poses[i], seeds[i]) for i in range(len(des_poses))]
    return {k: np.stack([r[k] for r in rows]) for k in rows[0]}


def seed_rows(seed, G, M, first, down, up):
    """the rows of the seeded forms: [G][M][D]; the difference, the product and the sum each rounded once"""
    D = len(down)
    a = np.arange(G)[:, None, None]
    b = (first + np.arange(M))[None, :, None]
    d = np.arange(D)[None, None, :]
    hi, lo, _, _ = R.uniforms(R.block(seed, RNG_IK, a, b, 0, d))
    u = np.where(R.is_sine(d) == 1, lo, hi).astype(np.float64) * 2.0 ** -53
    return np.ascontiguousarray(down + u * (up - down))


def clearance(orc, model, ro, fld, conf):
    """conf [M][D] against an OracleField (score_reference.oracle_sdf) -> (clearance [M], out_of_range [M], near_face
    [M]: centres within 1e-9 of a field face); (+inf, 0, 0) without a field"""
    M = conf.shape[0]
    if fld is None:
        return np.full(M, np.inf), np.zeros(M, dtype=np.int32), np.zeros(M, dtype=np.int64)
    S = model.nr_body_spheres()
    centers, _ = orc.sphere_centers(ro, conf)
    pts = np.ascontiguousarray(centers[:, :, :fld.dim]).reshape(-1, fld.dim)
    dist, _, inr = orc.sdf_query(fld.handle, pts)
    dist, inr = dist.reshape(M, S), inr.reshape(M, S).astype(bool)
    radius = np.asarray(model.flat()["sphere_radius"], dtype=np.float64).reshape(1, S)
    p = pts.reshape(M, S, fld.dim)
    near = (np.abs(p - fld.origin).min(axis=2) < 1e-9) | (np.abs(p - fld.upper).min(axis=2) < 1e-9)
    return np.where(inr, dist - radius, np.inf).min(axis=1), (~inr).sum(axis=1).astype(np.int32), near.sum(axis=1)


def goal_score(conf, near, weights):
    """[M]: the weighted distance to `near`, or the row index"""
    M, D = conf.shape
    if near is None:
        return np.arange(M, dtype=np.float64)
    w = np.ones(D) if weights is None else np.asarray(weights, dtype=np.float64)
    s = np.zeros(M)
    for d in range(D):   # ascending d
        df = conf[:, d] - near[d]
        s = s + w[d] * (df * df)
    return np.sqrt(s)


def goal_dist(conf, weights):
    """[M][M]: the MAX_STATE distance of "distinct alternatives" between rows of one state"""
    M, D = conf.shape
    w = np.ones(D) if weights is None else np.asarray(weights, dtype=np.float64)
    s = np.zeros((M, M))
    with np.errstate(invalid="ignore"):
        for d in range(D):
            df = conf[:, None, d] - conf[None, :, d]
            s = s + w[d] * (df * df)
        return np.sqrt(s)


def goals(conf, status, clr, oor, has_field, radius, max_goals, required_clearance=0.0, require_in_range=False,
          near=None, weights=None):
    """The goal stage of one pose on given IK answers -> dict(eligible, score, mode, leaders, n_goals, n_converged,
    n_eligible, goal_seed [max_goals], margin): margin is the smallest |dist - radius| over the pairs the rule can read
    and |clearance - required| over the converged rows -- how far the decisions are from flipping."""
    el = status == CONVERGED
    if has_field:
        el = el & (clr >= required_clearance) & ((oor == 0) | (not require_in_range))
    score = goal_score(conf, near, weights)
    dist = goal_dist(conf, weights)
    mode, leaders, sizes, n = scoring.group_rule(dist, score, el.astype(np.int32), radius)
    seed = np.full(max_goals, -1, dtype=np.int32)
    k = min(n, max_goals)
    seed[:k] = leaders[:k]
    sub = dist[np.ix_(el, el)]
    margin = np.abs(sub - radius).min() if sub.size else np.inf
    return dict(eligible=el, score=score, mode=mode, leaders=leaders, n_goals=n, n_converged=int((status == CONVERGED).sum()),
                n_eligible=int(el.sum()), goal_seed=seed, margin=margin, dist=dist)


# ------------------------------------------------------------------------------------------------ the cases
@dataclass
class Case:
    name: str
    model: object
    opts: Opts
    G: int
    M: int
    seed: int          # of the seeded draw
    pose_seed: int     # of the configurations whose forward kinematics are the poses
    poses: np.ndarray = field(default=None)
    seeds: np.ndarray = field(default=None)


def planar1():
    """one revolute joint, link length 0.5, one sphere at the tip"""
    arm = g.Arm(1, [0.5], [0.0], [0.0])
    return g.ArmModel(arm, [g.BodySphere(0, 0.01, (0.0, 0.0, 0.0))])


def fk_pose(orc, ro, link, q):
    return orc.forward_kinematics(ro, np.asarray(q, dtype=np.float64).reshape(1, -1))[0][0, link]


def make_case(orc, name, model, mode, G, M, seed, pose_seed, down, up, **kw):
    D = model.dof()
    o = Opts(mode=mode, link=model.fk_model().nr_links() - 1, down=np.asarray(down, float), up=np.asarray(up, float), **kw)
    ro = orc.robot(model)
    rng = np.random.default_rng(pose_seed)
    poses = np.stack([fk_pose(orc, ro, o.link, o.down + rng.random(D) * (o.up - o.down)) for _ in range(G)])
    return Case(name, model, o, G, M, seed, pose_seed, poses, seed_rows(seed, G, M, 0, o.down, o.up))


def cases(orc):
    """the cases of tests/test_gpu_ik.py; WAM POSE carries 65 rows, of which M = 1, 63, 64 are prefixes (a row of the
    seeded draw does not depend on M)"""
    wam, pi = g.generateArm("WAMArm"), np.pi
    a2, a3 = g.generateArm("SimpleTwoLinksArm"), g.generateArm("SimpleThreeLinksArm")
    return [
        make_case(orc, "wam_pose", wam, POSE, 3, 65, 11, 101, WAM_DOWN, WAM_UP),
        make_case(orc, "wam_position", wam, POSITION, 1, 64, 12, 102, WAM_DOWN, WAM_UP),
        make_case(orc, "wam_orientation", wam, ORIENTATION, 1, 64, 13, 103, WAM_DOWN, WAM_UP),
        make_case(orc, "arm3_pose", a3, POSE, 2, 64, 14, 104, [-pi] * 3, [pi] * 3),
        make_case(orc, "arm2_position", a2, POSITION, 1, 64, 15, 105, [-pi] * 2, [pi] * 2),
        make_case(orc, "planar1_position", planar1(), POSITION, 1, 64, 16, 106, [-pi], [pi]),
    ]


def perturb(seeds, rng, ulps=2):
    """every coordinate moved by `ulps` ulp, up or down at random"""
    up = rng.integers(0, 2, size=seeds.shape).astype(bool)
    out = seeds.copy()
    for _ in range(ulps):
        out = np.where(up, np.nextafter(out, np.inf), np.nextafter(out, -np.inf))
    return out


def sensitivity(orc, case, ref, trials=4):
    """the reference against itself on seeds moved by +-2 ulp -> (d_self [G][M]: the largest move of a configuration
    over the trials, on rows converged both times; flips: rows whose status or iters changed in any trial)"""
    ro = orc.robot(case.model)
    rng = np.random.default_rng(case.seed + 1000)
    d_self = np.zeros((case.G, case.M))
    flips = np.zeros((case.G, case.M), dtype=bool)
    for _ in range(trials):
        alt = solve_all(orc, ro, case.opts, case.poses, perturb(case.seeds, rng))
        flips |= (alt["status"] != ref["status"]) | (alt["iters"] != ref["iters"])
        both = (alt["status"] == CONVERGED) & (ref["status"] == CONVERGED)
        d = np.abs(alt["conf"] - ref["conf"]).max(axis=2)
        d_self = np.maximum(d_self, np.where(both, d, 0.0))
    return d_self, flips


_CACHE = {}


def reference(orc):
    """every case with its reference run and its sensitivity, computed once per process:
    list of (case, ref, d_self, flips)"""
    if "all" not in _CACHE:
        out = []
        for c in cases(orc):
            ref = solve_all(orc, orc.robot(c.model), c.opts, c.poses, c.seeds)
            d_self, flips = sensitivity(orc, c, ref)
            out.append((c, ref, d_self, flips))
        _CACHE["all"] = out
    return _CACHE["all"]
