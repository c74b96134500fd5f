"""The self-collision check of include/gpmp2mi.h ("self-collision check") restated in numpy on the CPU oracle:
interpolate_traj -> sphere_centers -> pair distances, radii from the model; and the list rule with a parent table per
robot kind written down here, independently of the library's.  Shared by tests/test_self_cpu.py (oracle only) and
tests/test_gpu_self.py (the expectation of the device's scores)."""
import numpy as np

from gpmp2_amd import robots

import score_reference as ref


def link_parents(model):
    """parent of every link of the model's kinematic tree (-1: the root), by robot kind"""
    fk = model.fk_model()
    L = fk.nr_links()
    par = [l - 1 for l in range(L)]                      # arms and one-arm mobile kinds: a chain from link 0
    if isinstance(fk, robots.Pose2Mobile2Arms):          # vehicle 0; arm 1: 1 .. a1; arm 2: a1 + 1 ..
        par[1 + fk.arm1.dof()] = 0
    elif isinstance(fk, robots.Pose2MobileVetLin2Arms):  # vehicle 0, torso 1; arm 1: 2 .. a1 + 1; arm 2: a1 + 2 ..
        par[2 + fk.arm1.dof()] = 1
    return par


def joint_distance(par, a, b):
    """number of joints between links a and b of the tree"""
    def chain(l):
        out = [l]
        while par[l] >= 0:
            l = par[l]
            out.append(l)
        return out
    ca, cb = chain(a), chain(b)
    common = next(l for l in ca if l in cb)
    return ca.index(common) + cb.index(common)


def candidate_pairs(model, min_joint_gap):
    """[P][2] int: all sphere pairs A < B, lexicographic, whose links are at least min_joint_gap joints apart"""
    if isinstance(model.fk_model(), robots.PointRobot):
        return np.zeros((0, 2), dtype=np.int64)
    par = link_parents(model)
    link = [s.link_id for s in model.spheres]
    S = len(link)
    out = [(a, b) for a in range(S) for b in range(a + 1, S) if joint_distance(par, link[a], link[b]) >= min_joint_gap]
    return np.array(out, dtype=np.int64).reshape(-1, 2)


def pair_clearance(model, centers, ids, epsilon=0.0):
    """centers [M][S][3], ids [P][2] -> (dist [M][P], total_eps [P]); clearance = dist - total_eps"""
    radius = np.asarray(model.flat()["sphere_radius"], dtype=np.float64)
    a, b = ids[:, 0].astype(int), ids[:, 1].astype(int)
    d = centers[:, a, :] - centers[:, b, :]
    with np.errstate(invalid="ignore", over="ignore"):
        dist = np.sqrt((d * d).sum(axis=2))
    return dist, radius[a] + radius[b] + epsilon


def generated_table(orc, model, ro, min_joint_gap=2, ref_conf=None, epsilon=0.0, sigma=1.0):
    """the table gpmp2mi_self_pairs_generate is specified to give, [P][4]"""
    ids = candidate_pairs(model, min_joint_gap)
    if ref_conf is not None and len(ids):
        q = np.ascontiguousarray(ref_conf, dtype=np.float64).reshape(-1, model.dof())
        centers, _ = orc.sphere_centers(ro, q)
        dist, te = pair_clearance(model, centers, ids)
        ids = ids[~((dist - te) < 0.0).any(axis=0)]
    t = np.zeros((len(ids), 4))
    t[:, :2], t[:, 2], t[:, 3] = ids, epsilon, sigma
    return t


def oracle_self_score(orc, model, ro, data, dt, inter_step, traj):
    """traj [B][N+1][2D], data [P][4] -> dict: the five per-row outputs plus what the comparisons need (gap: runner-up
    clearance minus the minimum per row; pairs: (state, pair)s per row; clearance [B][Md][P], +inf where invalid)."""
    D = model.dof()
    data = np.asarray(data, dtype=np.float64).reshape(-1, 4)
    P = data.shape[0]
    t = np.ascontiguousarray(traj, dtype=np.float64).reshape(-1, np.shape(traj)[-2], 2 * D)
    B = t.shape[0]
    with np.errstate(invalid="ignore"):
        U = orc.interpolate_traj(D, ref.is_lie(model), None, dt, inter_step, t)
    Md = U.shape[1]
    centers, _ = orc.sphere_centers(ro, np.ascontiguousarray(U[:, :, :D]).reshape(-1, D))
    dist, te = pair_clearance(model, centers, data[:, :2], data[:, 2])
    dist = dist.reshape(B, Md, P)
    valid = np.isfinite(dist)
    with np.errstate(invalid="ignore"):
        hinge = np.where(valid, np.where(dist > te, 0.0, te - dist), 0.0)
        clr = np.where(valid, dist - te, np.inf)
    flat = clr.reshape(B, Md * P)
    if Md * P == 0:
        mn, worst = np.full(B, np.inf), np.full((B, 2), -1, dtype=np.int32)
        gap = np.full(B, np.nan)
    else:
        arg = flat.argmin(axis=1)                 # first of equal minima: lowest state, then lowest pair
        mn = flat[np.arange(B), arg]
        worst = np.stack([arg // P, arg % P], axis=1).astype(np.int32)
        worst[~valid.reshape(B, -1).any(axis=1)] = -1
        part = np.partition(flat, 1, axis=1) if Md * P > 1 else np.full((B, 2), np.inf)
        with np.errstate(invalid="ignore"):
            gap = part[:, 1] - part[:, 0]
    return dict(self_support_cost=hinge[:, ::inter_step + 1].sum(axis=(1, 2)), self_dense_cost=hinge.sum(axis=(1, 2)),
                min_self_clearance=mn, worst=worst, invalid=(~valid).reshape(B, -1).sum(axis=1).astype(np.int32),
                gap=gap, pairs=Md * P, clearance=clr)


def close_rows(exp):
    """number of rows whose runner-up is within 1e-6 of the minimum: the rows a `worst` comparison may excuse"""
    with np.errstate(invalid="ignore"):
        return int((exp["gap"] <= 1e-6).sum())


def wam_table(orc, model, ro):
    """the 78 pairs of the WAM: links at least 2 joints apart, not touching at the zero configuration"""
    return generated_table(orc, model, ro, 2, np.zeros((1, model.dof())))


# ---------------------------------------------------------------------------------------------------------------------
# The inputs of tests/test_gpu_self.py, built without a GPU so that tests/test_self_cpu.py can judge them on the oracle.
DELTA_T = 0.25
TILE_EDGES = ((1, 0), (9, 6), (16, 3), (32, 3))      # (N, J): Md = 2, 64, 65, 129


def _planar_arm(n_per_link, radius):
    """3-link planar arm (links of 0.5) with n_per_link spheres spread over every link; radius: callable(i)"""
    arm = robots.Arm(3, [0.5, 0.5, 0.5], [0, 0, 0], [0, 0, 0])
    rows = [robots.BodySphere(l, radius(i), (-0.5 + 0.5 * (i + 0.5) / n_per_link, 0.0, 0.0))
            for l in range(3) for i in range(n_per_link)]
    return robots.RobotModel(arm, rows)


def models():
    import gpmp2_amd as g
    return dict(
        arm1=lambda: robots.RobotModel(robots.Arm(1, [0.5], [0], [0]), [robots.BodySphere(0, 0.05, (-0.25, 0.0, 0.0))]),
        # every coordinate a small dyadic number: the one distance is 5 exactly, in any arithmetic
        point2=lambda: robots.RobotModel(robots.PointRobot(2, 1), [robots.BodySphere(0, 0.5, (0.0, 0.0, 0.0)),
                                                                  robots.BodySphere(0, 0.75, (3.0, 4.0, 0.0))]),
        arm3s=lambda: _planar_arm(2, lambda i: 0.06),                       # S = 6: one wavefront
        arm3x96=lambda: _planar_arm(32, lambda i: 0.002 + 0.0001 * (i % 7)),  # S = 96: the LDS cap
        wam=lambda: g.generateArm("WAMArm"),
        config5=lambda: g.generateMobileArm("SimpleTwoLinksArm"),
        pr2=lambda: g.generateMobileArm("PR2"),
    )


def line_traj(rows, N, dt=DELTA_T):
    """rows: list of (start, end, amp) -> [B][N+1][2D]: start -> end with a sine bump of size amp, velocities to match"""
    out = []
    for start, end, amp in rows:
        start, end, amp = (np.asarray(x, dtype=np.float64) for x in (start, end, amp))
        i = np.arange(N + 1)[:, None] / N
        conf = start + (end - start) * i + np.sin(np.pi * i) * amp
        vel = ((end - start) + np.pi * np.cos(np.pi * i) * amp) / (N * dt)
        out.append(np.concatenate([conf, vel], axis=1))
    return np.ascontiguousarray(out)


FOLDED = ([0.10, np.pi - 0.05, np.pi + 0.03], [0.25, np.pi + 0.04, np.pi - 0.06], [0.0, 0.02, -0.02])
STRETCHED = ([0.2, 0.1, -0.1], [0.5, -0.2, 0.3], [0.1, 0.05, 0.0])


def case_traj(name, N):
    """the B = 3 rows of a case's robot"""
    rng = np.random.default_rng(7 + N)
    if name == "arm1":
        return line_traj([([0.0], [1.0], [0.2]), ([1.0], [-2.0], [0.0]), ([0.3], [0.4], [1.0])], N)
    if name == "point2":   # multiples of 1/8; exact only at support states, so this robot is scored with J = 0
        return line_traj([([-2.0, 1.0], [2.0, 3.0], [0.0, 0.0]), ([0.5, 0.25], [4.5, -3.75], [0.0, 0.0]),
                          ([1.0, 1.0], [1.0, 5.0], [0.0, 0.0])], N)
    if name == "arm3s":
        return line_traj([FOLDED, STRETCHED, ([0.3, 1.2, 2.0], [-0.4, 2.2, 1.1], [0.2, -0.3, 0.1])], N)
    if name == "arm3x96":
        return line_traj([([0.0, 2.55, 2.85], [0.3, 2.95, 2.45], [0.0, 0.0, 0.0]),
                          ([0.2, 2.9, 2.6], [0.1, 2.5, 3.0], [0.0, 0.0, 0.0]),
                          ([0.0, 2.4, -2.5], [0.5, 2.8, -2.9], [0.0, 0.0, 0.0])], N)
    if name == "wam":
        return line_traj([(rng.uniform(-1.5, 1.5, 7), rng.uniform(-1.5, 1.5, 7), rng.uniform(-0.5, 0.5, 7)) for _ in range(3)], N)
    if name == "config5":
        return line_traj([([-1.0, 0.0, 1.5, 0.2, 2.4], [1.0, 0.5, 0.9, 2.6, 2.9], [0.0, 0.3, 0.2, 0.3, -0.2]),
                          ([0.0, 0.0, 0.0, 3.0, 2.0], [0.5, -0.5, 1.0, 2.2, 3.0], [0.1, 0.0, 0.0, 0.0, 0.2]),
                          ([0.3, 0.2, -1.0, 0.1, 0.2], [-0.3, 0.6, 1.0, 0.9, -0.7], [0.0, 0.0, 0.5, 0.0, 0.0])], N)
    if name == "pr2":
        rows = []
        for b in range(3):
            start, end = np.zeros(18), np.zeros(18)
            start[:3], end[:3], end[3] = [-1.5, -1.0, 0.3], [1.5 - b, 1.2, -0.4], 0.2
            start[4:] = rng.uniform(-0.3, 0.3, 14)
            end[4:] = np.tile(np.linspace(0.2, 0.8, 7), 2) * np.r_[np.ones(7), -np.ones(7)] + rng.uniform(-0.4, 0.4, 14)
            rows.append((start, end, rng.normal(0, 0.15, 18)))
        return line_traj(rows, N)
    raise KeyError(name)


def case_table(name, which, orc, model, ro):
    """the pair table of a case: [P][4]"""
    S = model.nr_body_spheres()
    if which == "none":
        return np.zeros((0, 4))
    if which in ("generated", "generated3"):   # 3 joints apart: without the PR2's mirrored spheres two joints from a
        return generated_table(orc, model, ro, 3 if which == "generated3" else 2, np.zeros((1, model.dof())))   # sphere on their symmetry plane (ties by construction)
    if which == "all":
        ids = [(a, b) for a in range(S) for b in range(a + 1, S)]
    elif which == "base-hand":                  # WAM: the base sphere against three of the hand (fewer pairs than wavefronts)
        ids = [(0, 13), (14, 0), (0, 15)]
    elif which == "one":
        ids = [(1, 0)] if S == 2 else [tuple(candidate_pairs(model, 2)[-1])]
    else:                                       # an int: the last so many rows of the generated table, every other one reversed
        c = generated_table(orc, model, ro, 2, np.zeros((1, model.dof())))[-int(which):, :2].astype(int)
        ids = [tuple(c[i]) if i % 2 == 0 else tuple(c[i][::-1]) for i in range(int(which))]
    t = np.zeros((len(ids), 4))
    t[:, :2], t[:, 2], t[:, 3] = ids, 0.01 if name == "wam" else 0.0, 1.0
    return t


# (robot, table, (N, J)): every tile edge, every way the spheres and the pairs are shared
GPU_CASES = [("arm1", "none", (1, 0)), ("arm1", "none", (9, 6)), ("point2", "one", (1, 0)),
             ("arm3s", "one", (1, 0)), ("arm3s", 3, (9, 6)), ("arm3s", "generated", (16, 3)), ("arm3s", "all", (32, 3)),
             ("wam", "base-hand", (9, 6)), ("wam", 64, (16, 3)), ("wam", 65, (32, 3)), ("wam", "generated", (1, 0)),
             ("wam", "generated", (16, 3)), ("config5", "generated", (16, 3)), ("pr2", "generated3", (9, 6)),
             ("pr2", "generated3", (16, 3)), ("arm3x96", "all", (1, 0)), ("arm3x96", "all", (32, 3))]


def case_id(c):
    return f"{c[0]}-{c[1]}-N{c[2][0]}J{c[2][1]}"
