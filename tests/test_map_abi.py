"""Live map (include/gpmp2mi.h "live map") as far as it can be checked without a GPU: the ABI is declared and exported, the
argument errors that need no live handle are reported before the handle is looked at and before any device work, and the
Python wrappers refuse wrong shapes before the library is called.  What needs a live handle -- use_base without a base,
another device -- is in tests/test_gpu_map.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gpmp2_amd import _capi
from gpmp2_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_NAMES = ["gpmp2mi_sdf_reserve_update", "gpmp2mi_sdf_update", "gpmp2mi_sdf_update_dev",
             "gpmp2mi_sdf_update_from_occupancy", "gpmp2mi_sdf_update_from_occupancy_dev",
             "gpmp2mi_sdf_update_from_points", "gpmp2mi_sdf_update_from_points_dev", "gpmp2mi_multi_plan_refresh_field"]


@pytest.fixture(scope="module")
def eng():
    return E.Engine()


def test_entry_points_are_declared_and_exported(eng):
    hdr = open(os.path.join(ROOT, "include", "gpmp2mi.h")).read()
    assert "live map" in hdr
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for n in INT_NAMES:
        assert re.search(r"\bint\s+" + n + r"\s*\(", hdr), f"{n} is not declared in include/gpmp2mi.h"
        assert hasattr(eng.lib, n), f"{n} is not exported"


def test_bad_arguments_are_refused_before_the_handle_is_looked_at(eng):
    lib = eng.lib
    one = C.c_void_p(1)   # a non-null handle that must never be looked at: the bad argument is reported first
    vox, pts, conf = np.zeros(8), np.zeros((2, 3)), np.zeros(7)
    stats = np.full(4, 7, dtype=np.int32)
    v_, p_, q_, s_ = E.dptr(vox), E.dptr(pts), E.dptr(conf), E.iptr(stats)
    nan = float("nan")
    calls = {
        "reserve handle": lambda: lib.gpmp2mi_sdf_reserve_update(None),
        "update handle": lambda: lib.gpmp2mi_sdf_update(None, v_, 0),
        "update voxels": lambda: lib.gpmp2mi_sdf_update(one, None, 0),
        "update layout": lambda: lib.gpmp2mi_sdf_update(one, v_, 2),
        "update layout < 0": lambda: lib.gpmp2mi_sdf_update(one, v_, -1),
        "update_dev handle": lambda: lib.gpmp2mi_sdf_update_dev(None, one, None),
        "update_dev voxels": lambda: lib.gpmp2mi_sdf_update_dev(one, None, None),
        "occupancy handle": lambda: lib.gpmp2mi_sdf_update_from_occupancy(None, v_, 0),
        "occupancy occ": lambda: lib.gpmp2mi_sdf_update_from_occupancy(one, None, 0),
        "occupancy layout": lambda: lib.gpmp2mi_sdf_update_from_occupancy(one, v_, 7),
        "occupancy_dev handle": lambda: lib.gpmp2mi_sdf_update_from_occupancy_dev(None, one, None),
        "occupancy_dev occ": lambda: lib.gpmp2mi_sdf_update_from_occupancy_dev(one, None, None),
        "points handle": lambda: lib.gpmp2mi_sdf_update_from_points(None, 2, p_, 0, None, None, 0.0, s_),
        "points null": lambda: lib.gpmp2mi_sdf_update_from_points(one, 2, None, 0, None, None, 0.0, s_),
        "points M < 0": lambda: lib.gpmp2mi_sdf_update_from_points(one, -1, p_, 0, None, None, 0.0, s_),
        "points margin": lambda: lib.gpmp2mi_sdf_update_from_points(one, 2, p_, 0, None, None, nan, s_),
        "points conf": lambda: lib.gpmp2mi_sdf_update_from_points(one, 2, p_, 0, one, None, 0.0, s_),
        "points_dev handle": lambda: lib.gpmp2mi_sdf_update_from_points_dev(None, 2, one, 0, None, None, 0.0, None, None),
        "points_dev null": lambda: lib.gpmp2mi_sdf_update_from_points_dev(one, 2, None, 0, None, None, 0.0, None, None),
        "points_dev M < 0": lambda: lib.gpmp2mi_sdf_update_from_points_dev(one, -1, one, 0, None, None, 0.0, None, None),
        "points_dev margin": lambda: lib.gpmp2mi_sdf_update_from_points_dev(one, 2, one, 0, None, None, nan, None, None),
        "points_dev conf": lambda: lib.gpmp2mi_sdf_update_from_points_dev(one, 2, one, 0, one, None, 0.0, None, None),
        "refresh handle": lambda: lib.gpmp2mi_multi_plan_refresh_field(None),
    }
    for name, call in calls.items():
        assert call() == 1, name
        assert len(lib.gpmp2mi_last_error()) > 0, name
    assert stats.tolist() == [7, 7, 7, 7]       # a refused call writes nothing


def test_python_wrappers_refuse_bad_input_before_the_library_is_called():
    class Boom:
        def __getattr__(self, name):
            raise AssertionError(f"the library was called ({name})")

    class Field:
        ptr, dim, shape = None, 3, (4, 5, 6)

    class Robot:
        ptr, dof, S = None, 7, 16

    eng = E.Engine.__new__(E.Engine)
    eng.lib = Boom()
    s, r = Field(), Robot()
    for bad in (np.zeros((4, 5, 7)), np.zeros((6, 5, 4)), np.zeros(120), np.zeros((4, 5))):
        with pytest.raises(ValueError):
            eng.sdf_update(s, bad)
        with pytest.raises(ValueError):
            eng.sdf_update_from_occupancy(s, bad)
    with pytest.raises(ValueError):
        eng.sdf_update(s, np.zeros((4, 5, 6)), layout=2)
    for bad in (np.zeros((5, 2)), np.zeros(6), np.zeros((2, 3, 3))):
        with pytest.raises(ValueError):
            eng.sdf_update_from_points(s, bad)
    good = np.zeros((5, 3))
    with pytest.raises(ValueError):
        eng.sdf_update_from_points(s, good, robot=r)                          # a robot without its configuration
    with pytest.raises(ValueError):
        eng.sdf_update_from_points(s, good, robot=r, conf=np.zeros(6))
    with pytest.raises(ValueError):
        eng.sdf_update_from_points(s, good, margin=float("nan"))
    with pytest.raises(ValueError):
        eng.sdf_update_from_points_dev(s, -1, 1)
    with pytest.raises(ValueError):
        eng.sdf_update_from_points_dev(s, 5, 1, robot=r)
    with pytest.raises(ValueError):
        eng.sdf_update_from_points_dev(s, 5, 1, margin=float("nan"))
    planar = Field()
    planar.dim, planar.shape = 2, (5, 6)
    with pytest.raises(ValueError):
        eng.sdf_update_from_points(planar, good)
    with pytest.raises(ValueError):
        eng.sdf_update(planar, np.zeros((6, 5)))
