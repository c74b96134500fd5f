"""The re-timing rule of include/gpmp2mi.h ("re-timing") restated in numpy float64: the path derivatives of a trajectory,
the caps, the controllable sets, the greedy pass, the stamps and `achieved`.  Every expression is written in the order
of the header, so that on the same arrays the sets and rates are the bits of csrc/retime_rule.h (numpy rounds every
operation once).  Nothing here imports the product for its answers.  Shared by tests/test_retime_cpu.py (against the rule
built by the host compiler), tests/test_gpu_retime.py (the expectation of the device) and scripts/retime_error.py."""
import numpy as np

OK, BOUNDARY, EMPTY, INVALID = range(4)
INF = np.inf


def gp_coef(dt, tau):
    """(l21, l22, p21, p22) of the linear GP interpolator at tau inside an interval of dt: the velocity row"""
    a1, r = 0.5 * tau * tau, dt - tau
    w0, w1, w3 = 12.0 / (dt * dt * dt), -6.0 / (dt * dt), 4.0 / dt
    t2, t3 = a1 + tau * r, tau
    p21, p22 = t2 * w0 + t3 * w1, t2 * w1 + t3 * w3
    return -p21, 1.0 - (p21 * dt + p22), p21, p22


def path_from_traj(t, dt, J):
    """One trajectory t [N+1][2D] -> (qd, qdd_left, qdd_right [Md][D], h): q' of every checked state, q'' from the left
    and from the right (0 where there is no such side)."""
    t = np.asarray(t, dtype=np.float64)
    N, D = t.shape[0] - 1, t.shape[1] // 2
    J1 = J + 1
    Md, h = N * J1 + 1, dt / float(J1)
    x0, v0, x1, v1 = t[:-1, :D], t[:-1, D:], t[1:, :D], t[1:, D:]
    with np.errstate(invalid="ignore", over="ignore"):
        w = 6.0 / (dt * dt)
        wx = w * (x1 - x0)
        a0 = wx - (4.0 * v0 + 2.0 * v1) / dt
        a1 = -wx + (2.0 * v0 + 4.0 * v1) / dt
        qd, qL, qR = np.zeros((Md, D)), np.zeros((Md, D)), np.zeros((Md, D))
        for j in range(J1):
            sl = slice(j, N * J1, J1)
            if j == 0:
                qd[sl], qR[sl] = v0, a0
                continue
            l21, l22, p21, p22 = gp_coef(dt, float(j) * h)
            qd[sl] = l21 * x0 + l22 * v0 + p21 * x1 + p22 * v1
            qR[sl] = a0 + (a1 - a0) * (float(j) / float(J1))
            qL[sl] = qR[sl]
        qd[-1] = t[-1, D:]
        qL[J1::J1] = a1
    return qd, qL, qR, h


def rate_caps(qd, vel=None, ps=None, point_speed=INF):
    """[Md]: min_d (vel_d / |q'_d|)^2 and (point_speed / ps)^2; a zero denominator or an infinite limit caps nothing"""
    cap = np.full(qd.shape[0], INF)
    with np.errstate(divide="ignore", invalid="ignore"):
        if vel is not None:
            a = np.abs(qd)
            r = np.asarray(vel, dtype=np.float64) / a
            c = np.where((a == 0) | ~(np.asarray(vel) < INF), INF, r * r)
            cap = np.minimum(cap, np.where(np.isnan(c), INF, c).min(axis=1))
        if ps is not None and point_speed < INF:
            r = point_speed / np.abs(ps)
            cap = np.minimum(cap, np.where(np.abs(ps) == 0, INF, np.where(np.isnan(r), INF, r * r)))
    return cap


def _rows(k, qd, qL, qR, acc, h2, nlo, nhi):
    """(pl, pu, r, xcap) of the 2 D + 1 rows of stage k"""
    D = qd.shape[1]
    a = np.concatenate([qR[k], qL[k + 1]])
    b = np.concatenate([qd[k], qd[k + 1] + h2 * qL[k + 1]])
    A = np.concatenate([acc, acc])
    n = 2 * D + 1
    pl, pu, r, xcap = np.full(n, -INF), np.full(n, INF), np.zeros(n), np.full(n, INF)
    fin = A < INF
    z = fin & (b == 0) & (a != 0)
    nz = fin & (b != 0)
    xcap[:2 * D][z] = A[z] / np.abs(a[z])
    pu[:2 * D][nz] = A[nz] / np.abs(b[nz])
    pl[:2 * D][nz] = -pu[:2 * D][nz]
    r[:2 * D][nz] = -a[nz] / b[nz]
    pl[-1], pu[-1], r[-1] = nlo / h2, nhi / h2, -1.0 / h2
    return pl, pu, r, xcap


def retime_path(qd, qdd_left, qdd_right, cap, acc, h, max_rate=1.0, rate_start=None, rate_end=None, vel=None, ps=None,
                point_speed=INF):
    """One row -> dict(K [Md][2], x, sdot, u, stamps [Md], duration, status, achieved [4]).  vel / ps / point_speed:
    the limits `cap` was made from (the trajectory form's achieved[0] and [3]); without them achieved[0] is the cap
    ratio."""
    qd, qL, qR = (np.asarray(x, dtype=np.float64) for x in (qd, qdd_left, qdd_right))
    cap = np.asarray(cap, dtype=np.float64)
    Md, D = qd.shape
    acc = np.full(D, INF) if acc is None else np.asarray(acc, dtype=np.float64)
    h2 = 2.0 * h
    nan = np.full(Md, np.nan)
    res = dict(K=np.full((Md, 2), np.nan), x=nan.copy(), sdot=nan.copy(), u=nan.copy(), stamps=nan.copy(),
               duration=INF, status=OK, achieved=np.full(4, np.nan))

    def fail(status):
        res["status"] = status
        return res
    bad = ~np.isfinite(qd).all() or ~np.isfinite(qL[1:]).all() or ~np.isfinite(qR[:-1]).all() or not (cap >= 0).all()
    if ps is not None:
        bad = bad or not np.isfinite(ps).all()
    if bad:
        return fail(INVALID)
    X = np.minimum(cap, max_rate * max_rate)
    K = res["K"]
    lo, hi = 0.0, X[-1]
    if rate_end is not None:
        lo = rate_end * rate_end
        if lo > hi:
            return fail(BOUNDARY)
        hi = lo
    K[-1] = lo, hi
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for k in range(Md - 2, -1, -1):
            pl, pu, r, xcap = _rows(k, qd, qL, qR, acc, h2, lo, hi)
            al = r[:, None] - r[None, :]              # lower i, upper j
            be = pu[None, :] - pl[:, None]
            q = be / al
            t = min(X[k], xcap.min(), q[al > 0].min(initial=INF))
            lo_k = max(0.0, q[al < 0].max(initial=0.0))
            if ((al == 0) & (be < 0)).any() or lo_k > t:
                return fail(EMPTY)
            lo, hi = lo_k, t
            K[k] = lo, hi
        x, u = np.zeros(Md), np.zeros(Md)
        x[0] = hi
        if rate_start is not None:
            x[0] = rate_start * rate_start
            if x[0] < lo or x[0] > hi:
                return fail(BOUNDARY)
        for k in range(Md - 1):
            pl, pu, r, _ = _rows(k, qd, qL, qR, acc, h2, K[k + 1, 0], K[k + 1, 1])
            uh = (pu + r * x[k]).min()
            y = min(max(x[k] + h2 * uh, K[k + 1, 0]), K[k + 1, 1])
            x[k + 1] = y
            u[k] = (y - x[k]) / h2
        sdot = np.sqrt(x)
        den = sdot[:-1] + sdot[1:]
        if (den == 0).any():
            return fail(EMPTY)
        stamps = np.zeros(Md)
        for k in range(Md - 1):
            stamps[k + 1] = stamps[k] + h2 / den[k]
        res.update(x=x, sdot=sdot, u=u, stamps=stamps, duration=stamps[-1],
                   achieved=achieved(qd, qL, qR, cap, acc, h, x, u, vel, ps, point_speed))
    return res


def achieved(qd, qL, qR, cap, acc, h, x, u, vel=None, ps=None, point_speed=INF):
    """[4]: the largest ratios of a profile (x, u) by the definitions of the header"""
    h2 = 2.0 * h
    sdot = np.sqrt(x)
    fin = acc < INF
    xs, us = x[:-1, None], u[:-1, None]
    out = np.zeros(4)
    with np.errstate(divide="ignore", invalid="ignore"):
        e0 = np.abs(qR[:-1] * xs + qd[:-1] * us) / acc
        e1 = np.abs(qL[1:] * xs + (qd[1:] + h2 * qL[1:]) * us) / acc
        am = 0.5 * (qR[:-1] + qL[1:])
        vm = qd[:-1] + (0.5 * h) * qR[:-1] + (0.125 * h) * (qL[1:] - qR[:-1])
        em = np.abs(am * (xs + h * us) + vm * us) / acc
        if fin.any():
            out[1] = max(e0[:, fin].max(), e1[:, fin].max())
            out[2] = em[:, fin].max()
        if vel is None and ps is None:
            c = (cap < INF) & (cap > 0)
            if c.any():
                out[0] = (sdot[c] / np.sqrt(cap[c])).max()
        else:
            v = np.full(qd.shape[1], INF) if vel is None else np.asarray(vel, dtype=np.float64)
            if (v < INF).any():
                out[0] = (np.abs(qd) * sdot[:, None] / v)[:, v < INF].max()
            if ps is not None and point_speed < INF:
                out[3] = (ps * sdot / point_speed).max()
    return out


def retime_traj(t, dt, J, vel=None, acc=None, point_speed=INF, ps=None, max_rate=1.0, rate_start=None, rate_end=None):
    """One trajectory t [N+1][2D] with its sphere speeds ps [Md] (None: no Cartesian limit is asked) -> the dict of
    retime_path plus dense velocities (q' sdot) [Md][D]."""
    qd, qL, qR, h = path_from_traj(t, dt, J)
    D = qd.shape[1]
    v = np.full(D, INF) if vel is None else np.asarray(vel, dtype=np.float64)
    psk = np.zeros(qd.shape[0]) if ps is None else np.asarray(ps, dtype=np.float64)
    cap = rate_caps(qd, v, psk, point_speed)
    r = retime_path(qd, qL, qR, cap, acc, h, max_rate, rate_start, rate_end, v, psk, point_speed)
    r["vel_retimed"] = qd * r["sdot"][:, None]
    return r


def uniform_scale(qd, qL, qR, vel, acc, ps=None, point_speed=INF):
    """time_scale of "motion limits" from the same path derivatives: max(vel ratio, sqrt(acc ratio at the interval ends),
    ps / point_speed).  (q'' is linear inside an interval, so its extremes over all checked states are at the ends.)"""
    D = qd.shape[1]
    v = np.full(D, INF) if vel is None else np.asarray(vel, dtype=np.float64)
    a = np.full(D, INF) if acc is None else np.asarray(acc, dtype=np.float64)
    s = float((np.abs(qd) / v).max())
    s = max(s, float(np.sqrt(max((np.abs(qL[1:]) / a).max(), (np.abs(qR[:-1]) / a).max()))))
    if ps is not None and point_speed < INF:
        s = max(s, float(np.max(ps)) / point_speed)
    return s


# ---------------------------------------------------------------------------------------------------------------------
# Inputs.  Small trajectories in the manner of the prototype: a straight line plus a sine bump, velocities its finite
# difference plus noise; every other row starts and ends at rest; every fifth row pauses (two equal support states with
# zero velocity, so every b of the stage between them is 0).
def random_traj(rng, N, D, dt, rest=False, pause=False):
    s = np.linspace(0, 1, N + 1)[:, None]
    q = rng.normal(size=D) * s * 2 + 0.3 * np.sin(3 * s * rng.normal(size=D))
    v = np.gradient(q, dt, axis=0) + 0.05 * rng.normal(size=q.shape)
    if rest:
        v[0] = 0
        v[-1] = 0
    if pause and N > 3:
        q[2] = q[1]
        v[1] = 0
        v[2] = 0
    return np.ascontiguousarray(np.hstack([q, v]))


def path_cases():
    """list of (name, dict(traj, dt, J, vel, acc)): D 1-7, N 2-8, J 0-4, one with Md > 64, one with D = 18"""
    rng = np.random.default_rng(20240611)
    out = []
    for i in range(12):
        N, D, J = int(rng.integers(2, 9)), int(rng.integers(1, 8)), int(rng.integers(0, 5))
        if i % 5 == 0:
            N = max(N, 4)
        out.append((f"r{i}-D{D}N{N}J{J}", dict(traj=random_traj(rng, N, D, 0.5, rest=i % 2 == 0, pause=i % 5 == 0), dt=0.5,
                                                J=J, vel=np.full(D, 1.0) + 0.01 * np.arange(D), acc=np.full(D, 2.0))))
    out.append(("long-D3N20J4", dict(traj=random_traj(rng, 20, 3, 0.25, rest=True), dt=0.25, J=4, vel=np.full(3, 1.5),
                                     acc=np.full(3, 3.0))))
    out.append(("wide-D18N3J1", dict(traj=random_traj(rng, 3, 18, 0.5), dt=0.5, J=1, vel=np.full(18, 1.0),
                                     acc=np.full(18, 2.0) + 0.01 * np.arange(18))))
    acc = np.full(4, 2.0)
    acc[2] = INF
    out.append(("noacc-D4N5J2", dict(traj=random_traj(rng, 5, 4, 0.5, pause=True), dt=0.5, J=2, vel=None, acc=acc)))
    return out


def ulp_perturbed(t, rng, n=2):
    """t with every entry moved by up to n ulp.  Exact zeros stay: a trajectory at rest is a property of the input (its
    rows with b == 0), and two ulp of 0 would be a denormal velocity whose quotients overflow."""
    k = np.where(t == 0, 0, rng.integers(-n, n + 1, size=t.shape))
    out = t.copy()
    for s in range(1, n + 1):
        out = np.where(k >= s, np.nextafter(out, INF), np.where(k <= -s, np.nextafter(out, -INF), out))
    return out


def sphere_speeds(orc, model, ro, t, dt, J):
    """t [B][N+1][2D] -> ps [B][Md]: the largest sphere speed |J_s(q_k) v_k| of every checked state, on the CPU oracle's
    interpolation and Jacobians (fixed-base kinds)"""
    D, S = model.dof(), model.nr_body_spheres()
    t = np.ascontiguousarray(t, dtype=np.float64).reshape(-1, np.shape(t)[-2], 2 * D)
    with np.errstate(invalid="ignore", over="ignore"):
        U = orc.interpolate_traj(D, False, None, dt, J, t)
        q = np.ascontiguousarray(U[:, :, :D]).reshape(-1, D)
        _, Jc = orc.sphere_centers(ro, q)                                   # [M][S][3][D]
        u = (Jc * U[:, :, D:].reshape(-1, 1, 1, D)).sum(axis=3)
        return np.sqrt((u * u).sum(axis=2)).reshape(t.shape[0], U.shape[1], S).max(axis=2)
