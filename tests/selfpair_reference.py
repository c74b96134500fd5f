"""The self-collision table of a plan (include/gpmp2mi.h "self-collision table in a plan") restated in numpy on the CPU
oracle: the rows of oracle.self_collision_factor with a weight per pair, their normal-equation terms added to
oracle.linearize / graph_error, and a plain Gauss-Newton loop on oracle.block_tridiag_solve.  Shared by
tests/test_selfpair_cpu.py (oracle only) and tests/test_gpu_selfpair.py (the expectation of the device's results)."""
import numpy as np

from gpmp2_amd import robots

import moving_reference as mr
import score_reference as ref
import self_reference as sr


def _table(table):
    return np.ascontiguousarray(table, dtype=np.float64).reshape(-1, 4)


# ---------------------------------------------------------------------------------------------------- the factor
def rows(orc, model, ro, conf, table):
    """conf [M][D], table [P][4] -> err [M][P], H [M][P][D], dist [M][P]; dist == 0: err = total_eps and a zero row (the
    oracle divides by the distance there)"""
    D = model.dof()
    t = _table(table)
    q = np.ascontiguousarray(conf, dtype=np.float64).reshape(-1, D)
    with np.errstate(invalid="ignore", divide="ignore"):
        err, H = orc.self_collision_factor(ro, t, q)
    c, _ = orc.sphere_centers(ro, q)
    dist, _ = sr.pair_clearance(model, c, t[:, :2], t[:, 2])
    H = np.where((dist == 0.0)[..., None], 0.0, H)
    return err, H, dist


def plan_terms(orc, model, ro, traj, table, states):
    """traj [B][N+1][2D], states (first, last) -> G [B][N+1][D][D], g [B][N+1][D], e [B] (e = sum r^T r / 2), the rows
    whitened by the sigma of their pair"""
    D = model.dof()
    t = np.asarray(traj, dtype=np.float64)
    B, N1 = t.shape[0], t.shape[1]
    G, gg, e = np.zeros((B, N1, D, D)), np.zeros((B, N1, D)), np.zeros(B)
    tb = _table(table)
    if tb.shape[0] == 0:
        return G, gg, e
    first, last = states
    idx = np.arange(first, last + 1)
    err, H, _ = rows(orc, model, ro, t[:, idx, :D].reshape(-1, D), tb)
    r = err / tb[None, :, 3]
    A = H / tb[None, :, 3, None]
    G[:, idx] = np.einsum("mpa,mpb->mab", A, A).reshape(B, len(idx), D, D)
    gg[:, idx] = np.einsum("mpa,mp->ma", A, r).reshape(B, len(idx), D)
    e += 0.5 * (r * r).sum(axis=1).reshape(B, len(idx)).sum(axis=1)
    return G, gg, e


def _args(p):
    return p.start_conf, p.start_vel, p.end_conf, p.end_vel


def linearize(orc, ro, so, p, traj, sp):
    """oracle.linearize plus the table's terms on the configuration block of each state; sp: dict(table, states) or
    None"""
    Hd, Ho, gr, err = orc.linearize(ro, so, p.setting, *_args(p), traj)
    if sp is not None and len(sp["table"]):
        D = p.setting.dof
        G, gg, e = plan_terms(orc, p.model, ro, traj, sp["table"], sp["states"])
        Hd[:, :, :D, :D] += G
        gr[:, :, :D] += gg
        err = err + e
    return Hd, Ho, gr, err


def graph_error(orc, ro, so, p, traj, sp):
    err = orc.graph_error(ro, so, p.setting, *_args(p), traj)
    if sp is not None and len(sp["table"]):
        err = err + plan_terms(orc, p.model, ro, traj, sp["table"], sp["states"])[2]
    return err


def gauss_newton(orc, ro, so, p, sp, k, init=None):
    """the plain loop: x <- x + solve(H, -g), k times, for vector-space robots"""
    assert not ref.is_lie(p.model)
    x = np.array(p.init if init is None else init, dtype=np.float64)
    for _ in range(k):
        Hd, Ho, gr, _ = linearize(orc, ro, so, p, x, sp)
        dx, ok = orc.block_tridiag_solve(Hd, Ho, -gr)
        assert ok.all()
        x = x + dx
    return x


# ---------------------------------------------------------------------------------------------------------------------
# The inputs of tests/test_gpu_selfpair.py, built without a GPU so that tests/test_selfpair_cpu.py can judge them on the
# oracle.
EPSILON, SIGMA, ITERS = 0.05, 0.005, 5
SIGMAS = (0.01, 0.02, 0.05)
OFF = -10.0      # an epsilon that keeps a pair off in every state: total_eps < 0 <= dist
HINGE_MARGIN = 1e-8   # no |dist - total_eps| of a test table is below this: both sides take the same branch


def hinge_margin(orc, model, ro, traj, table):
    """the smallest |dist - total_eps| over the states of `traj` and the rows of `table`"""
    D = model.dof()
    t = np.asarray(traj, dtype=np.float64)
    tb = _table(table)
    c, _ = orc.sphere_centers(ro, np.ascontiguousarray(t[:, :, :D]).reshape(-1, D))
    dist, te = sr.pair_clearance(model, c, tb[:, :2], tb[:, 2])
    return float(np.abs(dist - te).min())


def near_table(orc, model, ro, traj, ids):
    """a table on `ids` [P][2] whose epsilon and sigma vary by row.  An even row's total_eps lies in the middle of the
    widest gap between the sorted distances of its pair over the states of `traj`, second and third quarter, so it is on
    in a quarter to three quarters of the states and no state sits on the edge of the hinge, where the last bit of a
    distance would decide (HINGE_MARGIN); a pair whose distance hardly changes (spheres two joints apart whose axes
    meet) is on in every state instead.  An odd row's total_eps is half its smallest distance: never on."""
    D = model.dof()
    t = np.asarray(traj, dtype=np.float64)
    c, _ = orc.sphere_centers(ro, np.ascontiguousarray(t[:, :, :D]).reshape(-1, D))
    dist, rr = sr.pair_clearance(model, c, ids)
    srt = np.sort(dist, axis=0)
    M = srt.shape[0]
    mid = srt[M // 4:3 * M // 4 + 1]
    j = np.diff(mid, axis=0).argmax(axis=0)
    cols = np.arange(len(ids))
    lo, hi = mid[j, cols], mid[j + 1, cols]
    on_some = np.where(hi - lo > 100 * HINGE_MARGIN, 0.5 * (lo + hi), 1.5 * srt[-1])
    te = np.where(cols % 2 == 0, on_some, 0.5 * srt[0])
    out = np.zeros((len(ids), 4))
    out[:, :2], out[:, 2] = ids, te - rr
    out[:, 3] = np.asarray(SIGMAS)[np.arange(len(ids)) % len(SIGMAS)]
    return out


def chunk_table(orc, model, ro, traj, ids, P=135):
    """P >= 130 rows by repeating `ids`: chunks 0 and 2 as near_table, the whole of chunk 1 (rows 64..127) off"""
    rep = ids[np.arange(P) % len(ids)]
    t = near_table(orc, model, ro, traj, rep)
    t[64:128, 2] = OFF
    return t


def chunk_activity(orc, model, ro, traj, table, states):
    """[chunks] bool: whether any (trajectory, state of the range, row of the chunk) is on"""
    D = model.dof()
    t = np.asarray(traj, dtype=np.float64)
    first, last = states
    err, _, _ = rows(orc, model, ro, t[:, first:last + 1, :D].reshape(-1, D), table)
    on = (err > 0).any(axis=0)
    return np.array([on[c:c + 64].any() for c in range(0, len(on), 64)])


def case_ids(name, model):
    """the pairs of a plan case: every pair whose links are at least two joints apart (78 + 1 on the WAM, more than
    1 000 on the PR2).  Pairs on neighbouring links are left out: config5 has two such spheres on one point."""
    return sr.candidate_pairs(model, 2)


WAM_SIZES = (1, 63, 64, 65)


def varied_pairs(orc, model, ro, traj, ids, P):
    """the P pairs of `ids` whose distance changes most over the states of `traj`, the widest range first"""
    D = model.dof()
    t = np.asarray(traj, dtype=np.float64)
    c, _ = orc.sphere_centers(ro, np.ascontiguousarray(t[:, :, :D]).reshape(-1, D))
    dist, _ = sr.pair_clearance(model, c, ids)
    return ids[np.argsort(-(dist.max(axis=0) - dist.min(axis=0)), kind="stable")[:P]]


def duplicated_sphere_model():
    """the WAM with its last sphere once more under a new id: the two centres are the same arithmetic on the same
    numbers, so they are equal bit for bit; -> (model, (A, B))"""
    import gpmp2_amd as g
    wam = g.generateArm("WAMArm")
    last = wam.spheres[-1]
    sph = list(wam.spheres) + [robots.BodySphere(last.link_id, last.radius, last.center)]
    return robots.RobotModel(wam.fk_model(), sph), (len(sph) - 2, len(sph) - 1)


def scenario():
    """mr.scenario()'s problem (WAM, B = 3, N = 10) for the solves with the 78-pair table"""
    return mr.scenario()[0]


def wam_table(orc, model, ro, epsilon=EPSILON, sigma=SIGMA):
    return sr.generated_table(orc, model, ro, 2, np.zeros((1, model.dof())), epsilon, sigma)
