"""The check stages of include/gpmp2mi.h (scoring, self-collision check, moving obstacles, carried object, workspace path,
motion limits, torque limits, re-timing, re-timing under torque limits) as one table: each stage's word in error messages and its per-row outputs in C argument
order.  The *_NAMES tuples of scoring.py, the validation of caller-supplied outputs, the pointer tuple of a host call
and the argument list of a `_dev` call (marshalling.py) all follow from it."""
from __future__ import annotations

from collections import namedtuple

import numpy as np

# outputs: (name, dtype, tail) with the array's shape [B] + tail(Md, D).  absent: what a form may go without, by name:
# "null" = the argument stays and takes NULL (the dict holds None), "dropped" = the form has no such argument (no key).
Stage = namedtuple("Stage", "word outputs absent")

_F, _I = np.float64, np.int32


def _row(Md, D):
    return ()


def _tail(*tail):
    return lambda Md, D: tail


def _stage(word, *outputs, **absent):
    return Stage(word, outputs, absent)


SCORE = _stage("score", ("support_cost", _F, _row), ("dense_cost", _F, _row), ("min_clearance", _F, _row),
               ("worst", _I, _tail(2)), ("out_of_range", _I, _row))
SELF = _stage("score", ("self_support_cost", _F, _row), ("self_dense_cost", _F, _row), ("min_self_clearance", _F, _row),
              ("worst", _I, _tail(2)), ("invalid", _I, _row))
MOVING = _stage("score", ("moving_support_cost", _F, _row), ("moving_dense_cost", _F, _row),
                ("min_moving_clearance", _F, _row), ("worst", _I, _tail(3)), ("invalid", _I, _row))
# not in STAGES: a stage of the same face as SCORE, against the carried set
CARRIED = _stage("score", ("carried_support_cost", _F, _row), ("carried_dense_cost", _F, _row),
                 ("min_carried_clearance", _F, _row), ("worst", _I, _tail(2)), ("out_of_range", _I, _row))
PATH = _stage("path", ("max_pos_dev", _F, _row), ("max_rot_dev", _F, _row), ("worst", _I, _tail(2)),
              ("support_cost", _F, _row), ("dense_cost", _F, _row), ("invalid", _I, _row))
MOTION = _stage("motion", ("pos_margin", _F, _row), ("vel_ratio", _F, _row), ("acc_ratio", _F, _row),
                ("point_speed", _F, _row), ("time_scale", _F, _row), ("worst", _I, _tail(4, 2)), ("invalid", _I, _row))
# tau: NULL when the torques themselves are not wanted
TORQUE = _stage("torque", ("torque_ratio", _F, _row), ("static_ratio", _F, _row), ("torque_time_scale", _F, _row),
                ("worst", _I, _tail(3, 2)), ("invalid", _I, _row), ("tau", _F, lambda Md, D: (Md, D)), tau="null")
# dense_retimed: not in the path form (gpmp2mi_retime_path), which has no robot
RETIME = _stage("retime", ("sdot", _F, lambda Md, D: (Md,)), ("u", _F, lambda Md, D: (Md,)),
                ("stamps", _F, lambda Md, D: (Md,)), ("duration", _F, _row), ("status", _I, _row),
                ("achieved", _F, _tail(4)), ("dense_retimed", _F, lambda Md, D: (Md, 2 * D)), dense_retimed="dropped")
# not in STAGES: re-timing under torque limits.  RETIME_AFFINE is the path form (gpmp2mi_retime_path_affine), which has no
# robot; RETIME_DYNAMIC the trajectory and plan forms, whose tau_retimed and coef take NULL when they are not wanted
RETIME_AFFINE = _stage("retime", *RETIME.outputs[:5], ("achieved", _F, _tail(6)))
RETIME_DYNAMIC = _stage("retime", *RETIME_AFFINE.outputs, RETIME.outputs[6], ("tau_retimed", _F, lambda Md, D: (Md, D)),
                        ("coef", _F, lambda Md, D: (Md, 4, D)), tau_retimed="null", coef="null")

STAGES = dict(score=SCORE, self=SELF, moving=MOVING, path=PATH, motion=MOTION, torque=TORQUE, retime=RETIME)


def names(stage):
    return tuple(name for name, _, _ in stage.outputs)


def shapes(stage, B, Md=None, D=None, absent=()):
    """(name, dtype, shape) of the outputs of one call, in C argument order, less the dropped ones among `absent`."""
    return [(name, dt, (B,) + tuple(tail(Md, D))) for name, dt, tail in stage.outputs
            if not (name in absent and stage.absent[name] == "dropped")]


def outputs(stage, B, Md=None, D=None, out=None, absent=()):
    """The per-row outputs of a call of `stage` as a dict in C argument order: fresh arrays, or the caller's (`out`, a
    dict with any of the names), checked for dtype, contiguity and shape.  absent: names of stage.absent this call goes
    without: a "null" one is None unless the caller brings the array, a "dropped" one is no output of the call."""
    res = {}
    out = out or {}
    want = shapes(stage, B, Md, D, absent)
    unknown = set(out) - {name for name, _, _ in want}
    if unknown:
        raise ValueError(f"unknown {stage.word} outputs: {sorted(unknown)}")
    for name, dt, shape in want:
        x = out.get(name)
        if x is None:
            x = None if name in absent else np.zeros(shape, dtype=dt)
        elif not isinstance(x, np.ndarray) or x.dtype != dt or not x.flags["C_CONTIGUOUS"] or x.shape != shape:
            raise ValueError(f"{name}: expected a contiguous {np.dtype(dt).name} array of shape {list(shape)}, got "
                             f"{getattr(x, 'dtype', type(x).__name__)} {list(np.shape(x))}")
        res[name] = x
    return res
