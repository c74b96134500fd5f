"""The posterior on the executed timeline (include/gpmp2mi.h), written once over a dtype: the covariance of every checked
state from the band of Sigma at the support states, the clearance deviation sigma(m, s) and the robust clearance.

    Sigma(m) = L S_ii L^T + P S_{i+1,i+1} P^T + P C L^T + (P C L^T)^T + Q_c(tau) (x) Qc        j > 0,  C = Sigma_{i+1,i}
    Sigma(m) = S_ii                                                                            j = 0
    h = grad d . d centre / d x,   sigma^2 = h Sigma_xx(m) h^T,   c_kappa = clearance - kappa sigma

L = Lambda_2(tau) (x) I, P = Psi_2(tau) (x) I are evaluated here in the dtype (the oracle's `gp_matrices` is their float64
form; tests/test_risk_cpu.py holds the two together).  The geometry -- checked configurations, sphere centres and their
Jacobians, field value and gradient -- is the oracle's (`interpolate_traj`, `sphere_centers`, `sdf_query`), in float64;
the band comes from `posterior_reference`.  In np.longdouble this is the truth the GPU tests compare against.

Two measures, per trajectory:

    e_cov = max |S^(m)_ab - S(m)_ab| / sqrt(S(m)_aa S(m)_bb)            over every entry of every checked state
    e_sig = max |sigma^^2 - sigma^2| / sbar^2,   sbar = sum_a |h_a| sqrt(Sigma_xx(m)_aa)       over the in-range pairs

sbar is the uncorrelated upper bound of sigma, so cancellation in h Sigma h^T cannot hide behind a relative measure;
pairs with sbar = 0 must give sigma^ = 0 exactly.
"""
from __future__ import annotations

import numpy as np

import posterior_reference as post

LD = np.longdouble


def gp_scalars(dt, tau, dtype=LD):
    """(Lambda_2, Psi_2), 2 x 2 each, of the constant-velocity GP with Qc factored out (gp/GPutils.h:44-59)"""
    dt, t = dtype(dt), dtype(tau)
    r = dt - t
    Qt = np.array([[t ** 3 / 3, t ** 2 / 2], [t ** 2 / 2, t]], dtype=dtype)
    Phr = np.array([[1, r], [0, 1]], dtype=dtype)
    Qinv = np.array([[12 / dt ** 3, -6 / dt ** 2], [-6 / dt ** 2, 4 / dt]], dtype=dtype)
    Psi = Qt @ Phr.T @ Qinv
    Lam = np.array([[1, t], [0, 1]], dtype=dtype) - Psi @ np.array([[1, dt], [0, 1]], dtype=dtype)
    return Lam, Psi


def qc_closed(dt, tau, dtype=LD):
    """the 2 x 2 conditional covariance of the prior bridge at tau, factored"""
    D, t = dtype(dt), dtype(tau)
    r = D - t
    q01 = t ** 2 * r ** 2 * (D - 2 * t) / (2 * D ** 3)
    return np.array([[t ** 3 * r ** 3 / (3 * D ** 3), q01], [q01, t * r * (D ** 2 - 3 * t * D + 3 * t ** 2) / D ** 3]], dtype=dtype)


def qc_subtractive(dt, tau, dtype=LD):
    """the same as Q(tau) - Psi_2 Q(dt) Psi_2^T"""
    D, t = dtype(dt), dtype(tau)
    Q = lambda x: np.array([[x ** 3 / 3, x ** 2 / 2], [x ** 2 / 2, x]], dtype=dtype)
    _, Psi = gp_scalars(dt, tau, dtype)
    return Q(t) - Psi @ Q(D) @ Psi.T


def dense_cov(Sd, So, Qc, dt, J, dtype=LD, slip=None):
    """band of one trajectory, Sd [N+1][n][n], So [N][n][n] -> cov [N (J+1) + 1][n][n] in `dtype`.
    slip = (m, rel): Psi_2[0][1] of checked state m is scaled by 1 + rel (the injected error of the CPU test)."""
    Sd, So = np.asarray(Sd, dtype=dtype), np.asarray(So, dtype=dtype)
    N, n = So.shape[0], Sd.shape[1]
    D = n // 2
    Qc = np.eye(D, dtype=dtype) if Qc is None else np.asarray(Qc, dtype=dtype)
    I = np.eye(D, dtype=dtype)
    cov = np.zeros((N * (J + 1) + 1, n, n), dtype=dtype)
    for i in range(N + 1):
        cov[i * (J + 1)] = Sd[i]
    for i in range(N):
        for j in range(1, J + 1):
            m = i * (J + 1) + j
            tau = dtype(j) * (dtype(dt) / dtype(J + 1))
            L2, P2 = gp_scalars(dt, tau, dtype)
            if slip is not None and slip[0] == m:
                P2 = P2.copy()
                P2[0, 1] *= 1 + dtype(slip[1])
            L, P = np.kron(L2, I), np.kron(P2, I)
            X = P @ So[i] @ L.T
            S = L @ Sd[i] @ L.T + P @ Sd[i + 1] @ P.T + X + X.T + np.kron(qc_closed(dt, tau, dtype), Qc)
            cov[m] = np.triu(S) + np.triu(S, 1).T      # symmetric, from one computed value
    return cov


def e_cov(cov_hat, cov):
    """correlation-scale error of one trajectory's dense blocks -> float"""
    cov = np.asarray(cov, dtype=LD)
    sg = np.sqrt(np.diagonal(cov, axis1=1, axis2=2))
    d = np.abs(np.asarray(cov_hat, dtype=LD) - cov)
    return float((d / (sg[:, :, None] * sg[:, None, :])).max())


def geometry(oracle, ro, so, model_lie, D, dt, J, traj, origin, cell):
    """the oracle's geometry of one trajectory [N+1][2D]: dict(clear [Md][S], h [Md][S][D], inr [Md][S] bool,
    near_face [Md][S] bool); clearance = dist - radius comes from the caller's radii (see `risk`)"""
    dense = oracle.interpolate_traj(D, int(model_lie), None, dt, J, traj[None])[0]
    conf = np.ascontiguousarray(dense[:, :D])
    c, Jc = oracle.sphere_centers(ro, conf)                       # [Md][S][3], [Md][S][3][D]
    Md, S = c.shape[0], c.shape[1]
    dim = so.dim
    dist, grad, inr = oracle.sdf_query(so, np.ascontiguousarray(c[:, :, :dim]).reshape(-1, dim))
    dist, grad, inr = dist.reshape(Md, S), grad.reshape(Md, S, dim), inr.reshape(Md, S).astype(bool)
    inr &= np.isfinite(c).all(axis=2)
    h = np.einsum("msk,mskd->msd", grad.astype(LD), Jc[:, :, :dim, :].astype(LD))
    h[~inr] = 0
    cells = (c[:, :, :dim] - np.asarray(origin, dtype=np.float64)[:dim]) / cell
    near = (np.abs(cells - np.round(cells)) < 1e-9).any(axis=2) & (np.abs(h) > 0).any(axis=2)
    return dict(dist=dist, h=h, inr=inr, near_face=near & inr)


def sigma_parts(geo, cov, D):
    """-> (sigma2 [Md][S], sbar [Md][S]) in long double from the geometry and the dense covariance of one trajectory"""
    Sxx = np.asarray(cov, dtype=LD)[:, :D, :D]
    h = geo["h"]
    s2 = np.einsum("msa,mab,msb->ms", h, Sxx, h)
    sbar = np.einsum("msa,ma->ms", np.abs(h), np.sqrt(np.maximum(np.diagonal(Sxx, axis1=1, axis2=2), 0)))
    return s2, sbar


def sig_errors(sigma_hat, s2, sbar):
    """|sigma^^2 - sigma^2| / sbar^2 per pair [Md][S] (long double); 0 where sbar = 0, NaN where sigma^ is NaN"""
    sh = np.asarray(sigma_hat, dtype=LD)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(sbar > 0, np.abs(sh ** 2 - s2) / sbar ** 2, LD(0))


def e_sig(sigma_hat, s2, sbar, use):
    """max |sigma^^2 - sigma^2| / sbar^2 over the pairs of `use` with sbar > 0; the others must be exactly 0 -> float"""
    sh = np.asarray(sigma_hat, dtype=LD)
    zero = use & (sbar == 0)
    assert np.all(sh[zero] == 0), "a pair with sbar = 0 has sigma != 0"
    pos = use & (sbar > 0)
    if not pos.any():
        return 0.0
    return float(sig_errors(sigma_hat, s2, sbar)[pos].max())


def robust(geo, radius, s2, kappa):
    """-> dict(c, worst (m, s), sigma_worst, gap to the runner-up, clear [Md][S], sigma [Md][S]) of one trajectory"""
    clear = geo["dist"].astype(LD) - np.asarray(radius, dtype=LD)[None, :]
    sg = np.sqrt(np.maximum(s2, 0))
    ck = np.where(geo["inr"], clear - LD(kappa) * sg, LD(np.inf))
    if not geo["inr"].any():
        return dict(c=np.inf, worst=(-1, -1), sigma_worst=0.0, gap=np.inf, clear=clear, sigma=sg, ck=ck)
    flat = np.argsort(ck.reshape(-1), kind="stable")
    m, s = np.unravel_index(flat[0], ck.shape)
    gap = float(ck.reshape(-1)[flat[1]] - ck.reshape(-1)[flat[0]]) if flat.size > 1 else np.inf
    return dict(c=float(ck[m, s]), worst=(int(m), int(s)), sigma_worst=float(sg[m, s]), gap=gap, clear=clear, sigma=sg,
                ck=ck)


def band_float64(Hd, Ho):
    """the two float64 bands of one linearization: the block recursion and the dense inverse"""
    return post.marginals(Hd, Ho, np.float64), post.dense_inv_band(Hd, Ho)
