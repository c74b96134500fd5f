"""The sampled clearance (include/gpmp2mi.h "sampled clearance"), written once on the CPU: the covariance of the prior
bridge over the sub-steps of an interval, and the pipeline of one row -- support samples, the configurations on the
executed timeline with the bridge noise, the clearance of every (sample, checked state), c_s, worst and the counts.

    delta = L^-T z,   z[i][rho] = normal(seed, POSTERIOR, r, q, i, rho)                     posterior_reference.sample
    zeta  = est + delta                                                                     one rounded addition
    x_s(m) = conf half of interpolate_traj(zeta)  [+ eps(i, j) for bridge and j > 0]        the oracle's interpolation
    eps(i, j) = sum_{j' <= j} Lp[j][j'] (C xi_{i,j'}),   xi[d] = normal(seed, BRIDGE, r, q, i (J+1) + j', d)
    P[a][b] = s^2 (D - t)^2 (3 t D - s D - 2 s t) / (6 D^3),  s = tau_a <= t = tau_b,   Lp Lp^T = P,  C C^T = Qc

The normals are those of rng_reference (float64, as the library makes them); the bridge matrix, its factor, C and the sum
are formed in np.longdouble; the geometry -- sphere centres and the field -- is the oracle's, in float64, at the rounded
configurations.  A plain module like risk_reference.py; tests/test_sampled_cpu.py pins it.
"""
from __future__ import annotations

import numpy as np

import posterior_reference as post
import rng_reference as rng

LD = np.longdouble
BRIDGE = 3
CAP = 1e-9           # the ceiling of the GPU bound (tests/test_gpu_sampled.py); tests/test_sampled_cpu.py holds it
T_MAP = 0.08         # the threshold of the state_hits checks


# ---------------------------------------------------------------------------------------------- the bridge
def taus(dt, J, dtype=LD):
    return np.array([dtype(j) * (dtype(dt) / dtype(J + 1)) for j in range(1, J + 1)], dtype=dtype)


def _Q(x, dtype):
    return np.array([[x ** 3 / 3, x ** 2 / 2], [x ** 2 / 2, x]], dtype=dtype)


def _Phi(x, dtype):
    return np.array([[1, x], [0, 1]], dtype=dtype)


def bridge_from_kernel(dt, J, dtype=LD):
    """P [J][J]: the position-position part of K0(s,t) - K0(s,D) Q(D)^-1 K0(D,t), K0(s,t) = Q(min) Phi(|t-s|)^T"""
    D = dtype(dt)
    t = taus(dt, J, dtype)
    Qinv = np.array([[12 / D ** 3, -6 / D ** 2], [-6 / D ** 2, 4 / D]], dtype=dtype)
    P = np.zeros((J, J), dtype=dtype)
    for a in range(J):
        for b in range(a, J):
            k_st = _Q(t[a], dtype) @ _Phi(t[b] - t[a], dtype).T                 # s = t[a] <= t = t[b]
            k_sD = _Q(t[a], dtype) @ _Phi(D - t[a], dtype).T
            k_Dt = (_Q(t[b], dtype) @ _Phi(D - t[b], dtype).T).T                # K0(D, t) = K0(t, D)^T
            P[a, b] = P[b, a] = (k_st - k_sD @ Qinv @ k_Dt)[0, 0]
    return P


def bridge_closed(dt, J, dtype=LD):
    D = dtype(dt)
    t = taus(dt, J, dtype)
    P = np.zeros((J, J), dtype=dtype)
    for a in range(J):
        for b in range(a, J):
            s, u = t[a], t[b]
            P[a, b] = P[b, a] = s ** 2 * (D - u) ** 2 * (3 * u * D - s * D - 2 * s * u) / (6 * D ** 3)
    return P


def chol_lower(A, dtype=LD):
    """row-wise Cholesky without pivoting, A = L L^T, in `dtype`; ValueError for a pivot that is not positive"""
    A = np.asarray(A, dtype=dtype)
    n = A.shape[0]
    L = np.zeros((n, n), dtype=dtype)
    for a in range(n):
        for b in range(a + 1):
            s = A[a, b] - (L[a, :b] * L[b, :b]).sum(dtype=dtype)
            if a == b:
                if not s > 0:
                    raise ValueError("a pivot is not positive")
                L[a, a] = np.sqrt(s)
            else:
                L[a, b] = s / L[b, b]
    return L


def bridge_factor(dt, J, dtype=LD):
    return chol_lower(bridge_closed(dt, J, dtype), dtype) if J > 0 else np.zeros((0, 0), dtype=dtype)


# ---------------------------------------------------------------------------------------------- samples
def support_samples(Hd, Ho, seed, r, q_first, K, dtype=np.float64):
    """delta [K][N+1][n] of global row r, samples q_first .., as float64 (computed in `dtype`)"""
    nb, n = np.shape(Hd)[0], np.shape(Hd)[1]
    z = rng.normal_fill(seed, rng.POSTERIOR, r, 1, q_first, K, nb, n)[0]
    return np.ascontiguousarray(post.sample(Hd, Ho, z, dtype).astype(np.float64))


def bridge_noise(Qc, D, dt, J, N, seed, r, q_first, K, Lp=None):
    """eps [K][Md][D] in long double: zero at the support states"""
    Md = N * (J + 1) + 1
    eps = np.zeros((K, Md, D), dtype=LD)
    if J == 0:
        return eps
    xi = rng.normal_fill(seed, BRIDGE, r, 1, q_first, K, Md, D)[0].astype(LD)          # [K][Md][D], block index = m
    C = chol_lower(np.eye(D) if Qc is None else Qc)
    eta = xi @ C.T
    Lp = bridge_factor(dt, J) if Lp is None else np.asarray(Lp, dtype=LD)
    inner = eta[:, :N * (J + 1)].reshape(K, N, J + 1, D)[:, :, 1:, :]                    # sub-steps 1 .. J
    parts = np.zeros((K, N, J + 1, D), dtype=LD)
    parts[:, :, 1:, :] = np.einsum("ab,knbd->knad", Lp, inner)
    eps[:, :N * (J + 1)] = parts.reshape(K, N * (J + 1), D)
    return eps


def configurations(oracle, D, dt, J, est, delta, eps=None):
    """x_s(m) [K][Md][D] in long double: the oracle's interpolation of zeta = est + delta (float64), plus eps"""
    zeta = np.asarray(est, dtype=np.float64)[None] + np.asarray(delta, dtype=np.float64)
    dense = oracle.interpolate_traj(D, 0, None, dt, J, np.ascontiguousarray(zeta))
    x = dense[:, :, :D].astype(LD)
    return x if eps is None else x + eps


def clearances(oracle, ro, fld, radius, conf):
    """conf [K][Md][D] -> (pair clearance [K][Md][S] with +inf out of range, in-range mask)"""
    K, Md, D = conf.shape
    c, _ = oracle.sphere_centers(ro, np.ascontiguousarray(np.asarray(conf, dtype=np.float64).reshape(-1, D)))
    S, dim = c.shape[1], fld.dim
    dist, _, inr = oracle.sdf_query(fld.handle, np.ascontiguousarray(c[:, :, :dim]).reshape(-1, dim))
    inr = inr.reshape(K, Md, S).astype(bool) & np.isfinite(c).all(axis=2).reshape(K, Md, S)
    clr = np.where(inr, dist.reshape(K, Md, S) - np.asarray(radius, dtype=np.float64)[None, None, :], np.inf)
    return clr, inr


def row(oracle, ro, fld, radius, Qc, D, dt, J, est, delta, seed, r, q_first, bridge=True, Lp=None):
    """the reference of one row for the K samples of `delta` [K][N+1][2D] -> dict(conf [K][Md][D] long double,
    state [K][Md], clearance [K], worst [K][2], oor [K] bool)"""
    K, N = delta.shape[0], delta.shape[1] - 1
    eps = bridge_noise(Qc, D, dt, J, N, seed, r, q_first, K, Lp) if bridge else None
    conf = configurations(oracle, D, dt, J, est, delta, eps)
    clr, inr = clearances(oracle, ro, fld, radius, conf)
    Md, S = clr.shape[1], clr.shape[2]
    state = clr.min(axis=2)
    flat = clr.reshape(K, Md * S)
    arg = flat.argmin(axis=1)                       # first of equal minima: lowest state, then lowest sphere
    worst = np.stack([arg // S, arg % S], axis=1).astype(np.int32)
    worst[~inr.reshape(K, -1).any(axis=1)] = -1
    return dict(conf=conf, state=state, clearance=flat[np.arange(K), arg], worst=worst,
                oor=(~inr).reshape(K, -1).any(axis=1))


def counts(state, T, bound=0.0):
    """state [K][Md] -> dict(hits, state_hits [Md]) at threshold T shifted by `bound`, and the undecided values"""
    c = state.min(axis=1)
    fin = np.isfinite(state)
    return dict(hits=int((c < T + bound).sum()), state_hits=(state < T + bound).sum(axis=0).astype(np.int32),
                undecided=int((fin & (np.abs(state - T) <= abs(bound))).sum()))


def t_med(clearance):
    """the midpoint of the two middle order statistics of c_s (K odd: the median and its upper neighbour)"""
    c = np.sort(np.asarray(clearance, dtype=np.float64))
    k = (c.size - 1) // 2
    return float(c[k]) if c.size == 1 else 0.5 * (float(c[k]) + float(c[k + 1]))


def map_errors(conf_hat, state_hat, ref):
    """(e_conf, e_clr) of a device answer against `ref` (the dict of `row`): max |conf - ref| and max |state - ref| over
    the finite entries; the inf patterns must agree"""
    e_conf = float(np.abs(np.asarray(conf_hat, dtype=LD) - ref["conf"]).max())
    fin = np.isfinite(ref["state"])
    assert np.array_equal(np.isposinf(state_hat), ~fin), "the +inf pattern of state_clearance differs"
    e_clr = float(np.abs(np.asarray(state_hat, dtype=LD)[fin] - ref["state"][fin].astype(LD)).max()) if fin.any() else 0.0
    return e_conf, e_clr
