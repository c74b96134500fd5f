"""The parity contract of SURVEY.md 8(d) -- identical iteration counts and status, final trajectory within 1e-6 of the
oracle -- and the one kind of exception it admits: a problem that amplifies last-bit differences by itself.

An exception is never excused by a wider gate.  It is MEASURED: the oracle is run against itself with its initial
values perturbed by +-2 ulp; if the oracle then differs from itself by d_self, two correct fp64 solvers cannot be
expected to agree better than a small multiple of that, and the GPU must stay within K_SELF * d_self.  A trajectory whose perturbed oracle run takes another
number of iterations counts as infinitely sensitive; such a trajectory must still show the same control flow on
the GPU as the unperturbed oracle."""
from __future__ import annotations

import os

import numpy as np

EPS = 2.0 ** -52
CONTRACT = 1e-6
K_SELF = 10.0   # measured: GPU-vs-oracle / oracle-vs-perturbed-oracle between 0.2 and 2.7 on every case above 1e-6
                # (profiles/r03_parity_sensitivity.txt, r03_case26_bisect.txt)


def _args(p):
    return p.start_conf, p.start_vel, p.end_conf, p.end_vel


def solve_both(engine, oracle, p, nthreads=None, forms=None):
    r, s = engine.robot(p.model), engine.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)
    ro, so = oracle.robot(p.model), oracle.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)
    nthreads = nthreads or min(os.cpu_count() or 1, 64)
    res = engine.batch_optimize(r, s, p.setting, *_args(p), p.init, forms=forms)
    ref = oracle.batch_optimize(ro, so, p.setting, *_args(p), p.init, nthreads=nthreads)
    return res, ref, (ro, so)


def per_traj_diff(a, b):
    B = a["traj"].shape[0]
    return np.abs(a["traj"] - b["traj"]).reshape(B, -1).max(axis=1)


def oracle_self_sensitivity(oracle, handles, p, ref, which=None, trials=4, seed=5, nthreads=None):
    """max over `trials` of |oracle(init * (1 +- 2 ulp)) - oracle(init)| per trajectory (inf where the perturbed run
    takes another number of iterations or ends with another status).  `which` = trajectory indices to probe."""
    ro, so = handles
    idx = np.arange(p.B) if which is None else np.asarray(which, dtype=int)
    if idx.size == 0:
        return np.zeros(0)
    nthreads = nthreads or min(os.cpu_count() or 1, 64)
    rng = np.random.default_rng(seed)
    sub = [np.ascontiguousarray(a[idx]) for a in _args(p)]
    init = np.ascontiguousarray(p.init[idx])
    d_self = np.zeros(idx.size)
    for _ in range(trials):
        init2 = init * (1.0 + 2 * EPS * rng.choice([-1.0, 1.0], size=init.shape))
        alt = oracle.batch_optimize(ro, so, p.setting, *sub, init2, nthreads=nthreads)
        same = (alt["iters"] == ref["iters"][idx]) & (alt["status"] == ref["status"][idx])
        dd = np.abs(alt["traj"] - ref["traj"][idx]).reshape(idx.size, -1).max(axis=1)
        d_self = np.maximum(d_self, np.where(same, dd, np.inf))
    return d_self


def check_contract(engine, oracle, p, label="", final_error_rtol=1e-9, trials=4, nthreads=None):
    """Asserts the contract for every trajectory of problem p and returns a report dict.  Trajectories above 1e-6 are
    admitted only inside K_SELF x the oracle's own 2-ulp sensitivity."""
    res, ref, handles = solve_both(engine, oracle, p, nthreads)
    assert list(res["iters"]) == list(ref["iters"]), (label, res["iters"], ref["iters"])
    assert list(res["status"]) == list(ref["status"]), (label, res["status"], ref["status"])
    d_gpu = per_traj_diff(res, ref)
    over = np.nonzero(d_gpu > CONTRACT)[0]
    d_self = np.zeros(p.B)
    if over.size:
        d_self[over] = oracle_self_sensitivity(oracle, handles, p, ref, over, trials=trials, nthreads=nthreads)
        bound = K_SELF * d_self[over]
        assert np.all(d_gpu[over] <= bound), (
            f"{label}: trajectories {over.tolist()} differ from the oracle by {d_gpu[over]} but the oracle's own 2-ulp "
            f"sensitivity there is only {d_self[over]}")
    # final error.  It is a deterministic function E(x) of the values a solve returns, so it is pinned in two steps:
    # the GPU's number must be the ORACLE's E at the GPU's own trajectory to 1e-9 (this checks the error arithmetic and
    # is free of any amplification), and the trajectories themselves are pinned above.  Where both sides returned the
    # same trajectory to ~1e-9 the two numbers are also compared directly.
    ro, so = handles
    e_at_gpu = oracle.graph_error(ro, so, p.setting, *_args(p), res["traj"])
    rel_own = np.abs(res["final_error"] / e_at_gpu - 1.0)
    assert np.all(rel_own <= final_error_rtol), (label, rel_own.max())
    rel = np.abs(res["final_error"] / ref["final_error"] - 1.0)
    same = d_gpu <= 1e-9 * np.maximum(np.abs(ref["traj"]).reshape(p.B, -1).max(axis=1), 1.0)
    assert np.all(rel[same] <= 10.0 * final_error_rtol), (label, rel[same].max())
    return dict(d_gpu=d_gpu, d_self=d_self, over=over, rel_err=rel, res=res, ref=ref)
