"""The score-and-select stage in numpy terms: the selection rule of include/gpmp2mi.h ("scoring") stated once, and the
shape checks of the wrappers in engine.py.  The scores themselves come from the device (k_score); nothing here computes
a collision cost."""
from __future__ import annotations

import numpy as np

TRAJ_NOT_SPD = 3   # GPMP2MI_TRAJ_NOT_SPD


def checked_states(total_step, inter_step):
    """Md: number of states the stage checks for a trajectory of total_step intervals."""
    return int(total_step) * (int(inter_step) + 1) + 1


def eligible(final_error, status, min_clearance, out_of_range, required_clearance=0.0, require_in_range=False,
             min_self_clearance=None, invalid=None, required_self_clearance=0.0):
    """Boolean mask [B] of the rows the rule may choose (status None: all fine; out_of_range None: all in range).
    min_self_clearance / invalid (include/gpmp2mi.h "self-collision check"): the row must also keep
    required_self_clearance from itself and have no invalid pair; None: not asked."""
    fe = np.asarray(final_error, dtype=np.float64).reshape(-1)
    clr = np.asarray(min_clearance, dtype=np.float64).reshape(-1)
    ok = np.isfinite(fe)
    if status is not None:
        ok &= np.asarray(status).reshape(-1) != TRAJ_NOT_SPD
    with np.errstate(invalid="ignore"):
        ok &= clr >= required_clearance          # False for a NaN clearance
    if require_in_range and out_of_range is not None:
        ok &= np.asarray(out_of_range).reshape(-1) == 0
    if min_self_clearance is not None:
        with np.errstate(invalid="ignore"):
            ok &= np.asarray(min_self_clearance, dtype=np.float64).reshape(-1) >= required_self_clearance
    if invalid is not None:
        ok &= np.asarray(invalid).reshape(-1) == 0
    return ok


def select_rule(final_error, status, min_clearance, out_of_range, required_clearance=0.0, require_in_range=False,
                min_self_clearance=None, invalid=None, required_self_clearance=0.0):
    """(best, n_eligible): the eligible row with the smallest final_error, the lowest row on ties; (-1, 0) if none."""
    fe = np.asarray(final_error, dtype=np.float64).reshape(-1)
    ok = eligible(fe, status, min_clearance, out_of_range, required_clearance, require_in_range, min_self_clearance,
                  invalid, required_self_clearance)
    rows = np.flatnonzero(ok)
    if rows.size == 0:
        return -1, 0
    return int(rows[np.argmin(fe[rows])]), int(rows.size)   # argmin returns the first of equal minima


def select_inputs(final_error, status, min_clearance, out_of_range, require_in_range):
    """The four arrays of a select_best call as contiguous float64 / int32 [B]; ValueError unless their lengths agree."""
    fe = np.ascontiguousarray(final_error, dtype=np.float64).reshape(-1)
    clr = np.ascontiguousarray(min_clearance, dtype=np.float64).reshape(-1)
    st = None if status is None else np.ascontiguousarray(status, dtype=np.int32).reshape(-1)
    oor = None if out_of_range is None else np.ascontiguousarray(out_of_range, dtype=np.int32).reshape(-1)
    B = fe.size
    for name, x in (("min_clearance", clr), ("status", st), ("out_of_range", oor)):
        if x is not None and x.size != B:
            raise ValueError(f"{name}: expected [{B}] like final_error, got [{x.size}]")
    if require_in_range and oor is None:
        raise ValueError("require_in_range needs out_of_range")
    return B, fe, st, clr, oor


def traj_rows(traj, D, total_step=None):
    """traj as contiguous float64 [B][N+1][2D] (a single [N+1][2D] trajectory becomes B = 1); ValueError otherwise."""
    t = np.ascontiguousarray(traj, dtype=np.float64)
    if t.ndim == 2:
        t = t[None]
    if t.ndim != 3 or t.shape[2] != 2 * D or t.shape[1] < 2 or (total_step is not None and t.shape[1] != total_step + 1):
        n = "N+1" if total_step is None else str(total_step + 1)
        raise ValueError(f"traj: expected [B][{n}][{2 * D}], got {list(np.shape(traj))}")
    return t


SCORE_NAMES = ("support_cost", "dense_cost", "min_clearance", "worst", "out_of_range")
SELF_NAMES = ("self_support_cost", "self_dense_cost", "min_self_clearance", "worst", "invalid")


def pair_table(data, S=None):
    """A pair table as contiguous float64 [P][4] (sphere A, sphere B, epsilon, sigma); [P][2] / [P][3] rows are completed
    with epsilon 0, sigma 1.  ValueError for another shape, or (S given) ids that are not distinct integers in [0, S)."""
    t = np.asarray(data, dtype=np.float64)
    if t.size == 0:
        return np.zeros((0, 4))
    if t.ndim != 2 or t.shape[1] not in (2, 3, 4):
        raise ValueError(f"pair table: expected [P][4], got {list(t.shape)}")
    full = np.zeros((t.shape[0], 4))
    full[:, 3] = 1.0
    full[:, :t.shape[1]] = t
    ids = full[:, :2]
    if S is not None and not ((ids == np.floor(ids)).all() and (ids >= 0).all() and (ids < S).all()
                              and (ids[:, 0] != ids[:, 1]).all()):
        raise ValueError(f"pair table: sphere ids must be distinct integers in [0, {S})")
    return np.ascontiguousarray(full)


def score_outputs(B, out=None, names=SCORE_NAMES):
    """The five per-row outputs of a score call: fresh arrays, or the caller's (a dict with any of the five names),
    checked for dtype, contiguity and length.  names: SCORE_NAMES, or SELF_NAMES for the self-collision check."""
    shapes = (((B,), np.float64), ((B,), np.float64), ((B,), np.float64), ((B, 2), np.int32), ((B,), np.int32))
    want = dict(zip(names, shapes))
    res = {}
    out = out or {}
    unknown = set(out) - set(want)
    if unknown:
        raise ValueError(f"unknown score outputs: {sorted(unknown)}")
    for name, (shape, dt) in want.items():
        x = out.get(name)
        if x is None:
            x = np.zeros(shape, dtype=dt)
        elif not isinstance(x, np.ndarray) or x.dtype != dt or not x.flags["C_CONTIGUOUS"] or x.shape != shape:
            raise ValueError(f"{name}: expected a contiguous {np.dtype(dt).name} array of shape {list(shape)}, got "
                             f"{getattr(x, 'dtype', type(x).__name__)} {list(np.shape(x))}")
        res[name] = x
    return res
