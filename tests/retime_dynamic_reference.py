"""The rule of include/gpmp2mi.h ("re-timing under torque limits") restated in numpy float64: the loop of
tests/retime_reference.py with affine rows |cx x + cu u + off| <= A next to its own, and the coefficients of the torque
rows tau = p u + m x + tau_g from tests/torque_reference.py::inverse_dynamics (link-frame two-pass; the device walks the
chain once in the world frame, so the two share no expression).  Every expression of the rule is written in the order
of csrc/retime_affine_rule.h, so that on the same arrays the sets and rates are its bits.  Nothing here imports the
product for its answers.  Shared by tests/test_retime_dynamic_cpu.py, tests/test_gpu_retime_dynamic.py and
scripts/retime_dynamic_error.py."""
import numpy as np

import retime_reference as rr
import torque_reference as tq

OK, BOUNDARY, EMPTY, INVALID, STATIC = range(5)
INF = np.inf
COEF = ("p", "m_left", "m_right", "tau_g")      # coef [..][4][D] in this order


def affine_rows(cx, cu, off, A):
    """(pl, pu, r, xcap) of the rows |cx x + cu u + off| <= A, arrays of one length"""
    cx, cu, off, A = (np.asarray(x, dtype=np.float64) for x in (cx, cu, off, A))
    n = cx.shape[0]
    pl, pu, r, xcap = np.full(n, -INF), np.full(n, INF), np.zeros(n), np.full(n, INF)
    fin = A < INF
    lo, hi = -A - off, A - off
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        pos, neg = fin & (cu > 0), fin & (cu < 0)
        pu[pos], pl[pos] = (hi / cu)[pos], (lo / cu)[pos]
        pu[neg], pl[neg] = (lo / cu)[neg], (hi / cu)[neg]
        nz = pos | neg
        r[nz] = (-cx / cu)[nz]
        z = fin & ~nz
        zp, zn = z & (cx > 0), z & (cx < 0)
        xcap[zp] = (hi / cx)[zp]
        xcap[zn] = (lo / cx)[zn]
    return pl, pu, r, xcap


def _rows(k, qd, qL, qR, acc, cxl, cxr, cu, off, bound, h2, nlo, nhi):
    """(pl, pu, r, xcap) of the 2 D + 2 R + 1 rows of stage k: those of retime_reference._rows, then the affine ones"""
    base = rr._rows(k, qd, qL, qR, acc, h2, nlo, nhi)
    start = affine_rows(cxr[k], cu[k], off[k], bound)
    end = affine_rows(cxl[k + 1], cu[k + 1] + h2 * cxl[k + 1], off[k + 1], bound)
    return tuple(np.concatenate([b, s, e]) for b, s, e in zip(base, start, end))


def retime_affine(qd, qdd_left, qdd_right, cap, acc, cx_left, cx_right, cu, off, bound, h, max_rate=1.0, rate_start=None,
                  rate_end=None, vel=None, ps=None, point_speed=INF):
    """One row -> dict(K [Md][2], x, sdot, u, stamps [Md], duration, status, achieved [6]): retime_reference.retime_path
    with R affine rows per state, cx_left, cx_right, cu, off [Md][R] and bound [R]."""
    qd, qL, qR = (np.asarray(x, dtype=np.float64) for x in (qd, qdd_left, qdd_right))
    cap = np.asarray(cap, dtype=np.float64)
    Md, D = qd.shape
    bound = np.asarray(bound, dtype=np.float64).reshape(-1)
    R = bound.shape[0]
    cxl, cxr, cu, off = (np.asarray(x, dtype=np.float64).reshape(Md, R) for x in (cx_left, cx_right, cu, off))
    acc = np.full(D, INF) if acc is None else np.asarray(acc, dtype=np.float64)
    h2 = 2.0 * h
    nan = np.full(Md, np.nan)
    res = dict(K=np.full((Md, 2), np.nan), x=nan.copy(), sdot=nan.copy(), u=nan.copy(), stamps=nan.copy(),
               duration=INF, status=OK, achieved=np.full(6, np.nan))

    def fail(status):
        res["status"] = status
        return res
    bad = ~np.isfinite(qd).all() or ~np.isfinite(qL[1:]).all() or ~np.isfinite(qR[:-1]).all() or not (cap >= 0).all()
    if ps is not None:
        bad = bad or not np.isfinite(ps).all()
    fin = bound < INF
    bad = bad or not (np.isfinite(cu[:, fin]).all() and np.isfinite(off[:, fin]).all()
                      and np.isfinite(cxl[1:, fin]).all() and np.isfinite(cxr[:-1, fin]).all())
    if bad:
        return fail(INVALID)
    if (np.abs(off[:, fin]) >= bound[fin]).any():
        return fail(STATIC)
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
            pl, pu, r, xcap = _rows(k, qd, qL, qR, acc, cxl, cxr, cu, off, bound, h2, lo, hi)
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
            pl, pu, r, _ = _rows(k, qd, qL, qR, acc, cxl, cxr, cu, off, bound, h2, K[k + 1, 0], K[k + 1, 1])
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
        ach = np.zeros(6)
        ach[:4] = rr.achieved(qd, qL, qR, cap, acc, h, x, u, vel, ps, point_speed)
        ach[4:] = achieved_affine(cxl, cxr, cu, off, bound, h, x, u)
        res.update(x=x, sdot=sdot, u=u, stamps=stamps, duration=stamps[-1], achieved=ach)
    return res


def affine_values(cxl, cxr, cu, off, h, x, u):
    """the affine rows at the start and at the end of every stage, [Md-1][R] each, from the profile (x, u)"""
    xs, us = x[:-1, None], u[:-1, None]
    return cxr[:-1] * xs + cu[:-1] * us + off[:-1], cxl[1:] * xs + (cu[1:] + (2.0 * h) * cxl[1:]) * us + off[1:]


def achieved_affine(cxl, cxr, cu, off, bound, h, x, u):
    """[2]: the largest |cx x + cu u + off| / bound over both ends of every stage, and the largest |off| / bound"""
    fin = bound < INF
    out = np.zeros(2)
    if fin.any():
        e0, e1 = affine_values(cxl, cxr, cu, off, h, x, u)
        out[0] = max((np.abs(e0) / bound)[:, fin].max(), (np.abs(e1) / bound)[:, fin].max())
        out[1] = (np.abs(off) / bound)[:, fin].max()
    return out


# ---------------------------------------------------------------------------------------------------------------------
# The coefficients of the torque rows
def coefficients(orc, model, table, dt, J, traj, dtype=np.float64):
    """traj [B][N+1][2D] -> coef [B][Md][4][D] = p, m_left, m_right, tau_g at every checked state (COEF): p = M(q) q' =
    ID(q, 0, q') without gravity, m = ID(q, q', q'') without gravity for the acceleration seen from the left and from the
    right (a state with one side: that side twice), tau_g = ID(q, 0, 0).  float64: on the oracle's interpolation; else
    the Hermite closed form in `dtype` (np.longdouble: the truth)."""
    arm, D = model.fk_model(), model.dof()
    U, first, second, has2 = tq.checked_inputs(orc, D, dt, J, traj, dtype)
    B, Md = U.shape[0], U.shape[1]
    q, v = U[:, :, :D].reshape(-1, D), U[:, :, D:].reshape(-1, D)
    zero = np.zeros_like(q)
    free = dict(table, gravity=np.zeros(3))
    left = np.where(has2[None, :, None], second, first)
    with np.errstate(invalid="ignore", over="ignore"):
        p = tq.inverse_dynamics(arm, free, q, zero, v, dtype)
        mR = tq.inverse_dynamics(arm, free, q, v, first.reshape(-1, D), dtype)
        mL = tq.inverse_dynamics(arm, free, q, v, left.reshape(-1, D), dtype)
        tg = tq.inverse_dynamics(arm, table, q, zero, zero, dtype)
    return np.stack([x.reshape(B, Md, D) for x in (p, mL, mR, tg)], axis=2)


def torque_limits(table, D):
    lim = table.get("torque")
    return np.full(D, INF) if lim is None else np.asarray(lim, dtype=np.float64)


def retime_dynamic_traj(t, coef, bound, dt, J, vel=None, acc=None, point_speed=INF, ps=None, max_rate=1.0,
                        rate_start=None, rate_end=None):
    """One trajectory t [N+1][2D] with its coefficients coef [Md][4][D] and torque limits bound [D] -> the dict of
    retime_affine plus vel_retimed [Md][D] and tau_retimed [Md][D] = m_{k+} x_k + p_k u_k + tau_g,k (the last state:
    m_- and u_{Md-2})."""
    qd, qL, qR, h = rr.path_from_traj(t, dt, J)
    D = qd.shape[1]
    v = np.full(D, INF) if vel is None else np.asarray(vel, dtype=np.float64)
    psk = np.zeros(qd.shape[0]) if ps is None else np.asarray(ps, dtype=np.float64)
    cap = rr.rate_caps(qd, v, psk, point_speed)
    c = np.asarray(coef, dtype=np.float64)
    r = retime_affine(qd, qL, qR, cap, acc, c[:, 1], c[:, 2], c[:, 0], c[:, 3], bound, h, max_rate, rate_start, rate_end,
                      v, psk, point_speed)
    r["vel_retimed"] = qd * r["sdot"][:, None]
    r["tau_retimed"] = tau_retimed(c, r["x"], r["u"])
    return r


def tau_retimed(coef, x, u):
    """[Md][D] from coef [Md][4][D] and the profile"""
    p, mL, mR, tg = (coef[:, i] for i in range(4))
    out = mR * x[:, None] + p * u[:, None] + tg
    out[-1] = mL[-1] * x[-1] + p[-1] * u[-2] + tg[-1]
    return out


def uniform_stretch(tref, qd, vel):
    """the uniform stretch of one row's duration that meets the torque and the speed limits: max(torque_time_scale, vel
    ratio), from torque_reference's score of the row (tref: its dict, one row) and the path derivatives"""
    v = np.full(qd.shape[1], INF) if vel is None else np.asarray(vel, dtype=np.float64)
    return max(float(tref), float((np.abs(qd) / v).max()))


def random_affine(rng, Md, R, static=False):
    """R affine rows per state with both signs of cu, a few cu == 0 (rows that cap x) and offsets inside the bound:
    (cx_left, cx_right, cu, off [Md][R], bound [R])"""
    bound = rng.uniform(2.0, 6.0, R)
    cxl, cxr = rng.normal(size=(Md, R)), rng.normal(size=(Md, R))
    cu = rng.normal(size=(Md, R)) * 2.0
    cu[rng.uniform(size=(Md, R)) < 0.1] = 0.0
    cxr[1::3] = cxl[1::3]                             # as inside an interval, where the two sides agree
    off = rng.uniform(-0.6, 0.6, (Md, R)) * bound
    if R > 1:
        bound[R // 2] = INF
    if static and R:
        off[Md // 2, 0] = -bound[0]
    return cxl, cxr, cu, off, bound
