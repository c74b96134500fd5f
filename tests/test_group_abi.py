"""The "distinct alternatives" section of include/gpmp2mi.h as far as it can be checked without a GPU: every name is
declared and exported, argument errors are reported before any device work and leave the outputs alone, and the Python
wrappers refuse misshaped arrays before the library is called."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gpmp2_amd import engine as E
from gpmp2_amd import scoring

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["gpmp2mi_traj_distances", "gpmp2mi_traj_distances_dev", "gpmp2mi_group_rows", "gpmp2mi_group_rows_dev",
         "gpmp2mi_group_traj", "gpmp2mi_group_traj_dev", "gpmp2mi_plan_select_distinct",
         "gpmp2mi_plan_select_distinct_dev"]
INF, NAN = float("inf"), float("nan")


@pytest.fixture(scope="module")
def eng():
    return E.Engine()


def test_entry_points_and_constants_are_declared_and_exported(eng):
    hdr = open(os.path.join(ROOT, "include", "gpmp2mi.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for n in NAMES:
        assert re.search(r"\bint\s+" + n + r"\s*\(", code), f"{n} is not declared in include/gpmp2mi.h"
        assert hasattr(eng.lib, n), f"{n} is not exported"
    assert re.search(r"GPMP2MI_DIST_MAX_STATE\s*=\s*0\s*,\s*GPMP2MI_DIST_RMS\s*=\s*1", code)
    assert re.search(r"#define\s+GPMP2MI_MAX_GROUP_ROWS\s+8192\b", code)
    assert re.search(r"#define\s+GPMP2MI_MAX_ALTERNATIVES\s+64\b", code)
    assert (scoring.MAX_GROUP_ROWS, scoring.MAX_ALTERNATIVES, scoring.DIST_MAX_STATE, scoring.DIST_RMS) == (8192, 64, 0, 1)
    # the section stands behind "self-collision check", counts the exception and says what is not here
    assert hdr.index("---- self-collision check") < hdr.index("---- distinct alternatives") < hdr.index("---- factor-level")
    section = hdr[hdr.index("---- distinct alternatives"):hdr.index("---- factor-level")]
    assert "sixth exception" in section and "No angle is wrapped" in section and "gpmp2mi_multi_plan_* twins" in section


def test_argument_errors_come_before_any_device_work_and_write_nothing(eng):
    lib = eng.lib
    one = C.c_void_p(1)                     # a non-null pointer that must never be looked at
    t, w = np.zeros((2, 3, 4)), np.ones(2)
    dist, sc = np.full((2, 2), 7.0), np.zeros(2)
    mode = np.full(2, 7, dtype=np.int32)
    n = C.c_int(7)
    d, i = E.dptr, E.iptr

    def distances(dof=2, B=2, N=2, traj=d(t), weights=None, metric=0, out=d(dist)):
        return lib.gpmp2mi_traj_distances(dof, B, N, traj, weights, metric, out)

    def group_traj(dof=2, B=2, N=2, traj=d(t), weights=None, metric=0, radius=1.0, score=d(sc)):
        return lib.gpmp2mi_group_traj(dof, B, N, traj, weights, metric, radius, score, None, i(mode), None, None, C.byref(n))

    def group_rows(B=2, dist_=d(dist), score=d(sc), radius=1.0):
        return lib.gpmp2mi_group_rows(B, dist_, score, None, radius, i(mode), None, None, C.byref(n))

    invalid = {
        "distances traj": lambda: distances(traj=None),
        "distances dist": lambda: distances(out=None),
        "distances B": lambda: distances(B=-1),
        "distances total_step": lambda: distances(N=0),
        "distances dof 0": lambda: distances(dof=0),
        "distances dof 19": lambda: distances(dof=19),
        "distances metric": lambda: distances(metric=2),
        "distances weight < 0": lambda: distances(weights=d(np.array([1.0, -1.0]))),
        "distances weight nan": lambda: distances(weights=d(np.array([NAN, 1.0]))),
        "distances weight inf": lambda: distances(weights=d(np.array([1.0, INF]))),
        "distances_dev traj": lambda: lib.gpmp2mi_traj_distances_dev(2, 2, 2, None, None, 0, one, None),
        "distances_dev dist": lambda: lib.gpmp2mi_traj_distances_dev(2, 2, 2, one, None, 0, None, None),
        "distances_dev metric": lambda: lib.gpmp2mi_traj_distances_dev(2, 2, 2, one, None, -1, one, None),
        "group_rows score": lambda: group_rows(score=None),
        "group_rows dist": lambda: group_rows(dist_=None),
        "group_rows B": lambda: group_rows(B=-1),
        "group_rows radius < 0": lambda: group_rows(radius=-1e-300),
        "group_rows radius nan": lambda: group_rows(radius=NAN),
        "group_rows_dev score": lambda: lib.gpmp2mi_group_rows_dev(2, one, None, None, 1.0, one, one, one, one, None),
        "group_rows_dev dist": lambda: lib.gpmp2mi_group_rows_dev(2, None, one, None, 1.0, one, one, one, one, None),
        "group_rows_dev radius": lambda: lib.gpmp2mi_group_rows_dev(2, one, one, None, NAN, one, one, one, one, None),
        "group_traj traj": lambda: group_traj(traj=None),
        "group_traj score": lambda: group_traj(score=None),
        "group_traj radius": lambda: group_traj(radius=-1.0),
        "group_traj metric": lambda: group_traj(metric=7),
        "group_traj weights": lambda: group_traj(weights=d(np.array([1.0, -0.5]))),
        "group_traj total_step": lambda: group_traj(N=0),
        "group_traj_dev traj": lambda: lib.gpmp2mi_group_traj_dev(2, 2, 2, None, None, 0, 1.0, one, None, one, one, one, one, None),
        "group_traj_dev score": lambda: lib.gpmp2mi_group_traj_dev(2, 2, 2, one, None, 0, 1.0, None, None, one, one, one, one, None),
        "group_traj_dev radius": lambda: lib.gpmp2mi_group_traj_dev(2, 2, 2, one, None, 0, NAN, one, None, one, one, one, one, None),
        "select_distinct plan": lambda: lib.gpmp2mi_plan_select_distinct(None, 0, 0.0, 0, None, 0.0, 0, None, 1.0, 4, C.byref(n),
                                                                         None, i(mode), None, None, None, None, None),
        "select_distinct_dev plan": lambda: lib.gpmp2mi_plan_select_distinct_dev(None, 0, 0.0, 0, None, 0.0, 0, None, 1.0, 4, one, one,
                                                                                 one, one, one, one, one, one, None),
    }
    for name, call in invalid.items():
        assert call() == 1, name
        assert len(lib.gpmp2mi_last_error()) > 0, name
    # more rows than the limit: unsupported, the limit named, through pointers that are never looked at
    big = scoring.MAX_GROUP_ROWS + 1
    unsupported = {
        "group_traj": lambda: lib.gpmp2mi_group_traj(2, big, 2, C.cast(one, E._capi.c_double_p), None, 0, 1.0,
                                                     C.cast(one, E._capi.c_double_p), None, i(mode), None, None, C.byref(n)),
        "group_traj_dev": lambda: lib.gpmp2mi_group_traj_dev(2, big, 2, one, None, 0, 1.0, one, None, one, one, one, one, None),
        "distances_dev": lambda: lib.gpmp2mi_traj_distances_dev(2, big, 2, one, None, 0, one, None),
        "group_rows_dev": lambda: lib.gpmp2mi_group_rows_dev(big, one, one, None, 1.0, one, one, one, one, None),
    }
    for name, call in unsupported.items():
        assert call() == 4, name
        assert b"8192" in lib.gpmp2mi_last_error(), name
    # a refused call writes nothing
    assert (dist == 7.0).all() and (mode == 7).all() and n.value == 7
    # B == 0 is fine and does nothing
    assert distances(B=0) == 0 and (dist == 7.0).all()
    assert group_traj(B=0) == 0 and n.value == 0
    n.value = 7
    assert group_rows(B=0, dist_=None) == 0 and n.value == 0


def test_python_wrappers_refuse_misshaped_arrays_before_the_library_is_called():
    class Boom:
        def __getattr__(self, name):
            raise AssertionError(f"the library was called ({name})")

    eng = E.Engine.__new__(E.Engine)
    eng.lib = Boom()
    good, sc = np.zeros((3, 5, 14)), np.zeros(3)
    for bad in (np.zeros((3, 5, 13)), np.zeros((3, 5)), np.zeros(14), np.zeros((3, 1, 14))):
        with pytest.raises(ValueError):
            eng.traj_distances(7, bad)
        with pytest.raises(ValueError):
            eng.group_traj(7, bad, sc, radius=1.0)
    for kw in (dict(weights=np.ones(6)), dict(weights=-np.ones(7)), dict(weights=np.full(7, NAN)), dict(metric=2),
               dict(metric="chebyshev")):
        with pytest.raises(ValueError):
            eng.traj_distances(7, good, **kw)
        with pytest.raises(ValueError):
            eng.group_traj(7, good, sc, radius=1.0, **kw)
    for kw in (dict(score=np.zeros(4)), dict(score=np.zeros((3, 1))), dict(score=sc, eligible=np.ones(2)),
               dict(score=sc, radius=-1.0), dict(score=sc, radius=NAN)):
        with pytest.raises(ValueError):
            eng.group_traj(7, good, **{"radius": 1.0, **kw})
    with pytest.raises(ValueError):
        eng.group_rows(np.zeros((3, 4)), sc, radius=1.0)
    with pytest.raises(ValueError):
        eng.group_rows(np.zeros((3, 3)), np.zeros(2), radius=1.0)
    with pytest.raises(ValueError):
        eng.group_rows(np.zeros((3, 3)), sc, eligible=np.ones(4), radius=1.0)
    with pytest.raises(ValueError):
        eng.group_rows(np.zeros((3, 3)), sc, radius=-0.5)
    with pytest.raises(ValueError):
        eng.group_traj_dev(7, scoring.MAX_GROUP_ROWS + 1, 4, 1, 1, radius=1.0)
    with pytest.raises(ValueError):
        eng.traj_distances_dev(7, 3, 4, 1, 1, weights=np.ones(3))
    pl = E.Plan.__new__(E.Plan)
    pl.eng, pl.B, pl.N, pl.D = eng, 2, 4, 7
    for args, kw in (((1, 1.0), dict(max_alt=0)), ((1, 1.0), dict(max_alt=65)), ((-1, 1.0), {}), ((1, -1.0), {}),
                     ((1, NAN), {}), ((1, 1.0), dict(weights=np.ones(3))), ((1, 1.0), dict(metric=5))):
        with pytest.raises(ValueError):
            pl.select_distinct(*args, **kw)
        with pytest.raises(ValueError):
            pl.select_distinct_dev(*args, **kw)
