"""The backward error of one optimizer step on the block-tridiagonal normal equations it claims to solve.

For a trajectory with diagonal blocks Hd[i], sub-diagonal blocks Ho[i] = block (i + 1, i) and gradient g, as
`linearize` returns them, and the step dx a solver took, in np.longdouble:

    r_i = sum_j H_ij dx_j + g_i                                          (block row i)
    eta = max_i |r_i|_inf / ( sum_j |H_ij|_inf |dx_j|_inf + |g_i|_inf )

Per block row on purpose: the position and velocity rows of Q^-1 differ by delta_t^-2, and one global norm would let an
error in a small block hide behind a large one.  A backward-stable solve keeps eta at a few units of roundoff whatever
the condition number; the forward error of the same solve grows with cond * eps, which is why the end-to-end parity
tests cannot see a slightly wrong elimination.  (The componentwise measure |r| / (|H| |dx| + |g|) is no use here: a
correct block Cholesky only reaches 1e-12 .. 3e-11 on it.)

The step is read back from the values: dx = after - before for vector-space robots, the local coordinates of `after`
at `before` for Pose2 robots.  The planner retracts a Pose2Vector with the first-order chart (compose with the increment
as a pose, no exponential map), so the local coordinates are `p2v_local`, the inverse of that chart, and not the
logarithm map.  Reading the step back costs one rounding of the values, |x| eps / |dx| relative to the step: part of
what eta measures, for the oracle and the engine alike.

A plain module like parity_bound.py; tests/test_backward_error_cpu.py pins the yardstick itself on the CPU oracle.
"""
from __future__ import annotations

import copy
import math

import numpy as np

LD = np.longdouble


# ---------------------------------------------------------------------------------------------- local coordinates
def p2v_local(a, b):
    """Pose2Vector localCoordinates(a -> b) in the first-order Pose2 chart (GTSAM default) on [x, y, theta], - on the
    rest."""
    a, b = np.asarray(a, float), np.asarray(b, float)
    c, s = math.cos(a[2]), math.sin(a[2])
    dx, dy = b[0] - a[0], b[1] - a[1]
    out = b - a
    out[0], out[1] = c * dx + s * dy, -s * dx + c * dy
    out[2] = math.atan2(math.sin(b[2] - a[2]), math.cos(b[2] - a[2]))
    return out


def local_coordinates(before, after, lie, near=None):
    """[..., 2D] states -> the step between them: after - before, and for a Pose2 robot (`lie`) p2v_local on the
    configuration half (the velocity half is a vector space).

    The heading of a Pose2 is kept in (-pi, pi], so a heading step is read back modulo 2 pi only -- and a first step
    from a poor initial guess can exceed pi (mobile_arm_config5 turns the base by -3.3 rad).  near: a step known to
    lie well within pi of the one taken (the reference solve of the same system); the heading step is then moved by
    the multiple of 2 pi that brings it closest to near's.  Both describe the same pose."""
    before, after = np.asarray(before, float), np.asarray(after, float)
    out = after - before
    if lie:
        D = before.shape[-1] // 2
        a, b, o = before.reshape(-1, 2 * D), after.reshape(-1, 2 * D), out.reshape(-1, 2 * D)
        for k in range(a.shape[0]):
            o[k, :D] = p2v_local(a[k, :D], b[k, :D])
        if near is not None:
            ref = np.asarray(near, float).reshape(-1, 2 * D)[:, 2]
            o[:, 2] += 2.0 * math.pi * np.round((ref - o[:, 2]) / (2.0 * math.pi))
    return out


def is_lie(model):
    return getattr(model, "kind", 0) >= 2


# ---------------------------------------------------------------------------------------------- the measure
def _inf_norm(M):
    """[..., n, n] -> matrix infinity norms (largest absolute row sum)"""
    return np.abs(M).sum(axis=-1).max(axis=-1)


def eta_block_rows(Hd, Ho, g, dx, lam=0.0):
    """One trajectory: Hd [nb][n][n], Ho [nb - 1][n][n], g [nb][n], dx [nb][n] -> eta of every block row, [nb]
    longdouble.  lam: Levenberg-Marquardt damping, added to the diagonal unscaled (as NormalEq::solve does).
    Walks the blocks; no dense matrix."""
    Hd, Ho, g, dx = (np.asarray(a, dtype=LD) for a in (Hd, Ho, g, dx))
    nb, n = g.shape
    assert Hd.shape == (nb, n, n) and Ho.shape == (max(nb - 1, 0), n, n) and dx.shape == (nb, n)
    if lam:
        Hd = Hd + LD(lam) * np.eye(n, dtype=LD)
    xn = np.abs(dx).max(axis=1)
    r = np.einsum("ijk,ik->ij", Hd, dx) + g
    den = _inf_norm(Hd) * xn + np.abs(g).max(axis=1)
    if nb > 1:
        r[1:] += np.einsum("ijk,ik->ij", Ho, dx[:-1])               # block (i + 1, i)
        den[1:] += _inf_norm(Ho) * xn[:-1]
        HoT = np.swapaxes(Ho, 1, 2)
        r[:-1] += np.einsum("ijk,ik->ij", HoT, dx[1:])              # block (i, i + 1) = Ho[i]^T
        den[:-1] += _inf_norm(HoT) * xn[1:]
    num = np.abs(r).max(axis=1)
    out = np.zeros(nb, dtype=LD)
    np.divide(num, den, out=out, where=den > 0)
    assert np.all((den > 0) | (num == 0)), "a block row with no scale and a residual"
    return out


def eta(Hd, Ho, g, dx, lam=0.0):
    """One trajectory -> eta (float)."""
    return float(eta_block_rows(Hd, Ho, g, dx, lam).max())


def eta_rows(Hd, Ho, g, dx, lam=0.0):
    """A batch ([B] leading on every array) -> eta per trajectory, [B] floats."""
    return np.array([eta(Hd[b], Ho[b], g[b], dx[b], lam) for b in range(np.shape(g)[0])])


# ---------------------------------------------------------------------------------------------- the step
def one_step_setting(setting, opt=None):
    """A copy of `setting` that takes exactly one iteration (fixed_iterations = 1); opt: "GN" / "LM" / "DOGLEG"."""
    st = copy.deepcopy(setting)
    st.fixed_iterations = 1
    if opt is not None:
        {"GN": st.setGaussNewton, "LM": st.setLM, "DOGLEG": st.setDogleg}[opt]()
    return st


def step_of(solver, before, lie, *solve, near=None, **kw):
    """The step a solver took from `before` ([B][N+1][2D]), in local coordinates.

    solver: a Plan that has already run (its result is read), or an Engine / the Oracle, which then runs
    batch_optimize(robot, sdf, setting, start_conf, start_vel, end_conf, end_vel) = *solve from `before` (forms=...
    is passed on); near: see local_coordinates.  -> (dx [B][N+1][2D], the result dict)."""
    before = np.asarray(before, float)
    res = solver.result() if hasattr(solver, "result") else solver.batch_optimize(*solve, before, **kw)
    return local_coordinates(before, res["traj"].reshape(before.shape), lie, near), res
