"""CPU-side checks of the seeding entry points (no GPU needed): they are declared in the public headers and exported
with the prototypes the Python bindings declare, refuse NULL plans and bad arguments before any device work, and the
wrapper refuses rows that disagree before anything reaches the library."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDING = ["gpmp2mi_normal_fill", "gpmp2mi_normal_fill_dev", "gpmp2mi_plan_seed_restarts",
           "gpmp2mi_plan_seed_restarts_dev", "gpmp2mi_plan_optimize_queue_seeded",
           "gpmp2mi_plan_optimize_queue_seeded_dev", "gpmp2mi_multi_plan_optimize_queue_seeded",
           "gpmp2mi_plan_sample_posterior_seeded", "gpmp2mi_plan_sample_posterior_seeded_dev"]
CTYPE = {"int": ctypes.c_int, "uint64_t": ctypes.c_uint64, "double": ctypes.c_double}


def _header(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def _params(text, name):
    """the parameter types of `int name(...)` in a header: 'ptr' for any pointer, else the scalar's ctypes type"""
    m = re.search(rf"\bint\s+{name}\s*\(([^)]*)\)", text)
    assert m, name
    out = []
    for par in m.group(1).split(","):
        par = par.strip()
        out.append("ptr" if "*" in par else CTYPE[par.replace("const ", "").split()[0]])
    return out


def test_seeding_entry_points_are_declared_exported_and_bound():
    from gpmp2_amd import engine
    text = _header("gpmp2mi.h")
    lib = engine.load_library()
    for name in SEEDING + ["gpmp2mi_debug_plan_seed_prior"]:
        want = _params(_header("gpmp2mi_debug.h") if "debug" in name else text, name)
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == len(want), name
        for k, (have, w) in enumerate(zip(fn.argtypes, want)):
            if w == "ptr":
                assert have is ctypes.c_void_p or issubclass(have, ctypes._Pointer), (name, k, have)
            else:
                assert have is w, (name, k, have, w)


def test_stream_ids_match_the_header_and_the_restatement():
    import rng_reference as rr
    from gpmp2_amd import _capi
    m = re.search(r"GPMP2MI_RNG_RESTARTS = (\d+), GPMP2MI_RNG_POSTERIOR = (\d+)", _header("gpmp2mi.h"))
    assert (int(m.group(1)), int(m.group(2))) == (_capi.RNG_RESTARTS, _capi.RNG_POSTERIOR) == (rr.RESTARTS, rr.POSTERIOR)


def test_null_plan_and_bad_fill_arguments_are_invalid():
    from gpmp2_amd import engine
    lib = engine.load_library()
    z = np.zeros(16)
    d = engine.dptr(z)
    assert lib.gpmp2mi_plan_seed_restarts(None, 1, 7, 0, 1.0, 0, d, d, None, d) == 1
    assert b"null plan" in lib.gpmp2mi_last_error()
    assert lib.gpmp2mi_plan_seed_restarts_dev(None, 1, 7, 0, 1.0, 0, 1, 1, None, 1, None) == 1
    assert lib.gpmp2mi_plan_optimize_queue_seeded(None, 1, 7, 0, 1.0, 0, d, d, d, d, None, None, None, None, None, None,
                                                  None) == 1
    assert lib.gpmp2mi_plan_optimize_queue_seeded_dev(None, 1, 7, 0, 1.0, 0, 1, 1, 1, 1, *[None] * 8) == 1
    assert lib.gpmp2mi_multi_plan_optimize_queue_seeded(None, 1, 7, 0, 1.0, 0, d, d, d, d, None, None, None, None, None,
                                                        None, None) == 1
    assert lib.gpmp2mi_plan_sample_posterior_seeded(None, 1, 7, 0, 0, d, None) == 1
    assert lib.gpmp2mi_plan_sample_posterior_seeded_dev(None, 1, 7, 0, 0, 1, None, None) == 1
    assert lib.gpmp2mi_debug_plan_seed_prior(None, d, d) == 1
    # the fill's arguments are checked before the device is touched
    assert lib.gpmp2mi_normal_fill(7, 1, 0, 1, 0, 1, 1, 17, d) == 1 and b"1..16" in lib.gpmp2mi_last_error()
    assert lib.gpmp2mi_normal_fill(7, 1, 0, 1, 0, 1, 1, 0, d) == 1
    assert lib.gpmp2mi_normal_fill(7, -1, 0, 1, 0, 1, 1, 4, d) == 1
    assert lib.gpmp2mi_normal_fill(7, 1 << 24, 0, 1, 0, 1, 1, 4, d) == 1
    assert lib.gpmp2mi_normal_fill(7, 1, 0, -1, 0, 1, 1, 4, d) == 1
    assert lib.gpmp2mi_normal_fill(7, 1, 0, 1, 0, 1, 1, 4, None) == 1
    assert lib.gpmp2mi_normal_fill(7, 1, 0, 0, 0, 1, 1, 4, d) == 0      # nothing to fill: no device needed


def test_wrapper_rejects_disagreeing_rows():
    from gpmp2_amd import engine
    D, N = 3, 4
    M, sc, ec, mu = engine.seed_inputs(D, N, np.zeros((5, D)), np.zeros((5, D)), None)
    assert M == 5 and mu is None
    M, sc, ec, mu = engine.seed_inputs(D, N, None, None, np.zeros((2, N + 1, 2 * D)), 2)
    assert M == 2 and sc is None and mu.shape == (2, N + 1, 2 * D)
    with pytest.raises(ValueError, match="disagree"):
        engine.seed_inputs(D, N, np.zeros((5, D)), np.zeros((4, D)), None)
    with pytest.raises(ValueError, match="disagree"):
        engine.seed_inputs(D, N, np.zeros((5, D)), np.zeros((5, D)), np.zeros((6, N + 1, 2 * D)))
    with pytest.raises(ValueError, match="disagree"):
        engine.seed_inputs(D, N, np.zeros((5, D)), np.zeros((5, D)), None, 4)
    with pytest.raises(ValueError, match="required"):
        engine.seed_inputs(D, N, None, np.zeros((5, D)), None)
