"""The posterior of a block-tridiagonal SPD system H, written once over a dtype: the blocks of Sigma = H^-1 on the band
(forward block Cholesky, backward Rauch-Tung-Striebel sweep) and the sampling solve delta = L^-T z (H = L L^T).

    forward    S_0 = H_00,  S_i = R_i^T R_i,  W_i = R_i^-T H_{i,i+1},  S_{i+1} = H_{i+1,i+1} - W_i^T W_i
    backward   G_i = R_i^-1 W_i,  Sigma_NN = R_N^-1 R_N^-T,  Sigma_{i,i+1} = -G_i Sigma_{i+1,i+1},
               Sigma_ii = R_i^-1 R_i^-T - Sigma_{i,i+1} G_i^T
    samples    Delta_N = R_N^-1 Z_N,  Delta_i = R_i^-1 (Z_i - W_i Delta_{i+1})

One trajectory at a time: Hd [nb][n][n], Ho [nb-1][n][n] = block (i+1, i), as `linearize` returns them.  In np.longdouble
this is the truth the GPU tests compare against (`truth`, `truth_sample`); in float64 it is one of the two yardsticks
(the other: np.linalg.inv of the dense matrix, `dense_inv_band`).

The measure is on correlation scale, per trajectory:

    e = max |Sigma^_ab - Sigma_ab| / sqrt(Sigma_aa Sigma_bb)      over every entry of every diagonal and off-diagonal block

The variances of a plan span 1e-8 (the states the priors hold) to 0.3, and an absolute or a global norm would hide the
tight states behind the loose ones.  For samples: max |delta^ - delta| / sigma, sigma = sqrt(diag Sigma).

A plain module like backward_error.py; tests/test_posterior_cpu.py pins the yardstick itself.
"""
from __future__ import annotations

import numpy as np

LD = np.longdouble


def _chol_upper(S):
    """S = R^T R, R upper triangular, in the dtype of S; ValueError for a pivot that is not positive"""
    n = S.shape[0]
    A, R = S.copy(), np.zeros_like(S)
    for j in range(n):
        if not A[j, j] > 0:
            raise ValueError("a pivot is not positive")
        R[j, j:] = A[j, j:] / np.sqrt(A[j, j])
        A[j + 1:, j + 1:] -= np.outer(R[j, j + 1:], R[j, j + 1:])
    return R


def _solve_upper(R, B):
    """R^-1 B by back-substitution"""
    X = np.zeros_like(B)
    for j in range(R.shape[0] - 1, -1, -1):
        X[j] = (B[j] - R[j, j + 1:] @ X[j + 1:]) / R[j, j]
    return X


def _solve_upper_t(R, B):
    """R^-T B by forward substitution"""
    X = np.zeros_like(B)
    for j in range(R.shape[0]):
        X[j] = (B[j] - R[:j, j] @ X[:j]) / R[j, j]
    return X


def _factor(Hd, Ho, dtype):
    """-> (R [nb][n][n], W [nb-1][n][n])"""
    Hd, Ho = np.asarray(Hd, dtype=dtype), np.asarray(Ho, dtype=dtype)
    nb, n = Hd.shape[0], Hd.shape[1]
    assert Hd.shape == (nb, n, n) and Ho.shape == (max(nb - 1, 0), n, n)
    R, W = np.zeros_like(Hd), np.zeros_like(Ho)
    S = Hd[0].copy()
    for i in range(nb):
        R[i] = _chol_upper(S)
        if i + 1 < nb:
            W[i] = _solve_upper_t(R[i], Ho[i].T.copy())     # H_{i,i+1} = Ho[i]^T
            S = Hd[i + 1] - W[i].T @ W[i]
    return R, W


def marginals(Hd, Ho, dtype=np.float64, slip=None):
    """-> (Sd [nb][n][n] = Sigma_ii, So [nb-1][n][n] = block (i+1, i) = Sigma_{i,i+1}^T) in `dtype`.
    slip = (i, r, c, rel): entry [r][c] of G_i is scaled by 1 + rel (the injected error of the CPU test)."""
    R, W = _factor(Hd, Ho, dtype)
    nb, n = R.shape[0], R.shape[1]
    eye = np.eye(n, dtype=dtype)
    Sd, So = np.zeros_like(R), np.zeros_like(W)
    Rinv = _solve_upper(R[-1], eye)
    Sd[-1] = Rinv @ Rinv.T
    for i in range(nb - 2, -1, -1):
        G, Rinv = _solve_upper(R[i], W[i]), _solve_upper(R[i], eye)
        if slip is not None and slip[0] == i:
            G[slip[1], slip[2]] *= 1 + dtype(slip[3])
        up = -G @ Sd[i + 1]                        # Sigma_{i,i+1}
        So[i] = up.T
        Sd[i] = Rinv @ Rinv.T - up @ G.T
    for i in range(nb):
        Sd[i] = np.triu(Sd[i]) + np.triu(Sd[i], 1).T   # symmetric, from one computed value
    return Sd, So


def sample(Hd, Ho, z, dtype=np.float64):
    """z [K][nb][n] -> delta [K][nb][n] = L^-T z in `dtype`"""
    R, W = _factor(Hd, Ho, dtype)
    z = np.asarray(z, dtype=dtype)
    nb = R.shape[0]
    d = np.zeros_like(z)
    d[:, -1] = _solve_upper(R[-1], z[:, -1].T.copy()).T
    for i in range(nb - 2, -1, -1):
        d[:, i] = _solve_upper(R[i], (z[:, i] - d[:, i + 1] @ W[i].T).T.copy()).T
    return d


def truth(Hd, Ho):
    assert np.finfo(LD).eps < 2e-19, "np.longdouble is not an extended type here: no truth to compare against"
    return marginals(Hd, Ho, LD)


def truth_sample(Hd, Ho, z):
    assert np.finfo(LD).eps < 2e-19, "np.longdouble is not an extended type here: no truth to compare against"
    return sample(Hd, Ho, z, LD)


def dense(Hd, Ho):
    """the dense symmetric matrix, in the dtype of Hd"""
    Hd, Ho = np.asarray(Hd), np.asarray(Ho)
    nb, n = Hd.shape[0], Hd.shape[1]
    H = np.zeros((nb * n, nb * n), dtype=Hd.dtype)
    for i in range(nb):
        H[i * n:(i + 1) * n, i * n:(i + 1) * n] = Hd[i]
        if i + 1 < nb:
            H[(i + 1) * n:(i + 2) * n, i * n:(i + 1) * n] = Ho[i]
            H[i * n:(i + 1) * n, (i + 1) * n:(i + 2) * n] = Ho[i].T
    return H


def band_of(S, nb, n):
    """dense [nb n][nb n] -> (Sd, So) as `marginals` returns them"""
    Sd = np.stack([S[i * n:(i + 1) * n, i * n:(i + 1) * n] for i in range(nb)])
    So = np.stack([S[(i + 1) * n:(i + 2) * n, i * n:(i + 1) * n] for i in range(nb - 1)]) if nb > 1 else \
        np.zeros((0, n, n), dtype=S.dtype)
    return Sd, So


def dense_inv_band(Hd, Ho):
    """the second float64 yardstick: np.linalg.inv of the dense matrix, its band"""
    Hd = np.asarray(Hd, dtype=np.float64)
    return band_of(np.linalg.inv(dense(Hd, np.asarray(Ho, dtype=np.float64))), Hd.shape[0], Hd.shape[1])


def sigma_of(Sd):
    """[nb][n][n] -> standard deviations [nb][n] (longdouble)"""
    return np.sqrt(np.diagonal(np.asarray(Sd, dtype=LD), axis1=1, axis2=2))


def cov_error(Sd_hat, So_hat, Sd, So):
    """e of one trajectory against the truth (Sd, So); any of the two estimates may be None -> float"""
    sg = sigma_of(Sd)
    e = LD(0)
    if Sd_hat is not None:
        d = np.abs(np.asarray(Sd_hat, dtype=LD) - np.asarray(Sd, dtype=LD))
        e = max(e, (d / (sg[:, :, None] * sg[:, None, :])).max())
    if So_hat is not None and np.shape(So)[0] > 0:
        d = np.abs(np.asarray(So_hat, dtype=LD) - np.asarray(So, dtype=LD))
        e = max(e, (d / (sg[1:, :, None] * sg[:-1, None, :])).max())     # block (i+1, i): rows of i+1, columns of i
    return float(e)


def sample_error(d_hat, d, Sd):
    """max |delta^ - delta| / sigma of one trajectory; d_hat, d [K][nb][n] -> float"""
    return float((np.abs(np.asarray(d_hat, dtype=LD) - np.asarray(d, dtype=LD)) / sigma_of(Sd)[None]).max())


def cpu_yardstick(Hd, Ho, tr=None):
    """e_cpu of one trajectory: the larger of the two float64 CPU values (block recursion, dense inv) against the truth"""
    tr = truth(Hd, Ho) if tr is None else tr
    return max(cov_error(*marginals(Hd, Ho, np.float64), *tr), cov_error(*dense_inv_band(Hd, Ho), *tr))
