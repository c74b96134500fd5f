"""Distinct alternatives on the device (include/gpmp2mi.h "distinct alternatives") against tests/group_reference.py:
all-pairs trajectory distances, the leader rule on synthetic modes, and the plan form on solved restarts.

The distance bound is derived, not measured: |d - d_ref| <= (n + 5) 2^-52 d_ref with n = D for MAX_STATE and
n = D (N+1) for RMS.  Every term w (x_b - x_c)^2 carries at most 3 roundings (difference, square, the multiply-add);
a sum of n non-negative terms adds n - 1 more; the division and the square root add fewer than 2 after the root
halves what came before; the factor 2 (2^-52 instead of the unit roundoff 2^-53) covers the float64 rounding of the
long-double reference itself.  All terms are non-negative, so relative errors do not grow in the sums or the max."""
import ctypes as C
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

import group_reference as gr
import score_reference as ref
from gpmp2_amd import engine as E
from gpmp2_amd import problems, scoring

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF, NAN = float("inf"), float("nan")
METRICS = (scoring.DIST_MAX_STATE, scoring.DIST_RMS)


def _chunk(D):
    """support states the pair kernel stages through LDS at a time (csrc/launch.h group_chunk_states)"""
    return max(1, 32 // D)


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


# one tile, the tile edge, the 2 x 2 and 3 x 3 triangles of tiles; N = 1, 2 and one just past the state chunk of D
# a tile tail together with a chunk tail at the widest and the narrowest row: (130, 2, 18), (130, 32, 1)
SHAPES = [(1, 1, 7), (2, 2, 18), (63, 1, 2), (64, 2, 1), (130, 2, 7), (130, 2, 18), (130, 32, 1)] + \
         [(65, N, D) for D in (1, 2, 7, 18) for N in sorted({1, 2, _chunk(D)})]


@pytest.mark.parametrize("shape", SHAPES, ids=[f"B{b}-N{n}-D{d}" for b, n, d in SHAPES])
def test_distances_match_the_long_double_reference(engine, shape):
    B, N, D = shape
    rng = np.random.default_rng(1000 * B + 10 * N + D)
    traj = gr.random_traj(rng, B, N, D)
    if B >= 2:
        traj[1] = traj[0]                               # a duplicated row
    w = rng.uniform(0.1, 3.0, D)
    w[rng.integers(0, D)] = 0.0
    for metric in METRICS:
        for weights in (None, w):
            got = engine.traj_distances(D, traj, weights, metric)
            want = gr.distances(traj, D, weights, metric)
            err = np.abs(got.astype(np.longdouble) - want)
            lim = gr.bound(want, D, N, metric)
            print(f"B={B} N={N} D={D} metric={metric} weights={'given' if weights is not None else 'NULL'}: "
                  f"max err / bound {float((err / np.where(lim > 0, lim, 1)).max()):.3f}")
            assert (err <= lim).all(), (metric, float(err.max()))
            assert np.array_equal(got, got.T) and np.array_equal(np.diag(got), np.zeros(B))
            if B >= 2:
                assert got[0, 1] == 0.0 and np.array_equal(got[0], got[1])
            # the float64 evaluation of the same formula stays inside the same bound
            assert (np.abs(gr.distances(traj, D, weights, metric, np.float64).astype(np.longdouble) - want) <= lim).all()


def test_a_pair_does_not_depend_on_the_batch_it_sits_in(engine):
    rng = np.random.default_rng(5)
    traj = gr.random_traj(rng, 130, 5, 7)
    rows = [3, 63, 64, 100, 129]
    for metric in METRICS:
        big = engine.traj_distances(7, traj, None, metric)
        small = engine.traj_distances(7, traj[rows], None, metric)
        assert np.array_equal(_bits(small), _bits(big[np.ix_(rows, rows)]))
        assert np.array_equal(_bits(big), _bits(engine.traj_distances(7, traj, None, metric)))      # twice in a row


def test_non_finite_rows_give_nan_where_the_arithmetic_does(engine):
    rng = np.random.default_rng(6)
    traj = gr.random_traj(rng, 70, 3, 2)
    clean = engine.traj_distances(2, traj, None, 0)
    traj[5, 1, 0] = NAN
    traj[66, 2, 1] = INF
    traj[7, 0, 3] = NAN                                  # a velocity: not read
    for metric in METRICS:
        got = engine.traj_distances(2, traj, None, metric)
        others = [b for b in range(70) if b not in (5, 66)]
        assert np.isnan(got[5]).all() and np.isnan(got[:, 5]).all()
        assert np.isnan(got[66, 66]) and np.isinf(got[66, others]).all() and np.array_equal(got, got.T, equal_nan=True)
        if metric == 0:
            assert np.array_equal(_bits(got[np.ix_(others, others)]), _bits(clean[np.ix_(others, others)]))
    # grouped: the NaN row leads a mode of its own, the inf row joins only at radius = inf
    g = engine.group_traj(2, traj, np.arange(70.0), None, INF)
    assert g["n_modes"] == 2 and list(g["leaders"][:2]) == [0, 5] and g["mode"][66] == 0 and g["sizes"][1] == 1


class _DevArray:
    """a device buffer from the library's own HIP runtime (gpmp2mi_debug_device_*): no second runtime in the process"""

    def __init__(self, engine, host, fill_byte=0x7B):
        self.eng, self.host = engine, np.ascontiguousarray(host).copy()
        self.p = C.c_void_p()
        engine._ck(engine.lib.gpmp2mi_debug_device_alloc(C.c_size_t(max(self.host.nbytes, 8)), fill_byte, C.byref(self.p)))
        if self.host.nbytes:
            engine._ck(engine.lib.gpmp2mi_debug_device_write(self.p, self.host.ctypes.data_as(C.c_void_p),
                                                             C.c_size_t(self.host.nbytes)))

    @property
    def ptr(self):
        return self.p.value

    def read(self):
        if self.host.nbytes:
            self.eng._ck(self.eng.lib.gpmp2mi_debug_device_read(self.host.ctypes.data_as(C.c_void_p), self.p,
                                                                C.c_size_t(self.host.nbytes)))
        return self.host.copy()

    def free(self):
        self.eng._ck(self.eng.lib.gpmp2mi_debug_device_free(self.p))


def _rows_dev(engine, dist, score, eligible, radius):
    """gpmp2mi_group_rows_dev on device copies of host arrays"""
    B = len(score)
    bufs = [_DevArray(engine, dist), _DevArray(engine, np.asarray(score, dtype=np.float64)),
            _DevArray(engine, np.asarray(eligible, dtype=np.int32))]
    outs = [_DevArray(engine, np.zeros(B, dtype=np.int32)) for _ in range(3)] + [_DevArray(engine, np.zeros(1, dtype=np.int32))]
    engine.group_rows_dev(B, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, radius, outs[0].ptr, outs[1].ptr, outs[2].ptr, outs[3].ptr)
    engine.traj_distances(1, np.zeros((1, 2, 2)))          # a host-pointer call: waits for the null stream
    got = dict(mode=outs[0].read(), leaders=outs[1].read(), sizes=outs[2].read(), n_modes=int(outs[3].read()[0]))
    for b in bufs + outs:
        b.free()
    return got


def _same_groups(a, b, what):
    for k in ("mode", "leaders", "sizes"):
        assert np.array_equal(a[k], b[k]), (what, k, a[k], b[k])
    assert a["n_modes"] == b["n_modes"], what


def _as_dict(t):
    return dict(mode=t[0], leaders=t[1], sizes=t[2], n_modes=t[3])


@pytest.mark.parametrize("G,B", [(1, 65), (3, 130), (7, 130)])
def test_grouping_of_synthetic_modes_equals_the_reference(engine, G, B):
    rng = np.random.default_rng(40 + G)
    N, D = 9, 7
    traj, which = gr.synthetic_modes(rng, G, B, N, D, delta=1e-3)
    score, eligible = gr.scores_with_ties(rng, B)
    for metric in METRICS:
        dref = gr.distances(traj, D, None, metric)
        radius = gr.gap_radius(dref)                      # asserts the gap condition on the reference
        want = _as_dict(gr.rule(dref, score, eligible, radius))
        got = engine.group_traj(D, traj, score, eligible, radius, None, metric)
        _same_groups(got, want, f"group_traj G={G} metric={metric}")
        if G > 1:                                         # the gap is the one between the bundles: the modes are the centres
            assert got["n_modes"] == len(set(which[(eligible != 0) & np.isfinite(score)]))
            part = got["mode"] >= 0
            assert (which[got["leaders"][got["mode"][part]]] == which[part]).all()
        dist = engine.traj_distances(D, traj, None, metric)
        _same_groups(engine.group_rows(dist, score, eligible, radius), got, "traj_distances + host group_rows")
        _same_groups(_rows_dev(engine, dist, score, eligible, radius), got, "traj_distances + group_rows_dev")
        _same_groups(_as_dict(scoring.group_rule(dist, score, eligible, radius)), got, "scoring.group_rule")


def test_radius_zero_radius_infinity_and_the_chain(engine):
    rng = np.random.default_rng(77)
    base = gr.random_traj(rng, 23, 4, 3)
    traj = base[rng.integers(0, 23, size=130)]            # 130 rows, 23 distinct ones: many rounds
    score = rng.permutation(130).astype(np.float64)
    dref = gr.distances(traj, 3)
    got = engine.group_traj(3, traj, score, None, 0.0)
    _same_groups(got, _as_dict(gr.rule(dref, score, None, 0.0)), "radius 0")
    assert got["n_modes"] == len(np.unique(traj.reshape(130, -1), axis=0)) == len(set(got["leaders"][:got["n_modes"]]))
    _same_groups(_rows_dev(engine, engine.traj_distances(3, traj), score, np.ones(130), 0.0), got, "radius 0, group_rows_dev")
    one = engine.group_traj(3, traj, score, None, INF)
    assert one["n_modes"] == 1 and one["leaders"][0] == int(np.argmin(score)) and one["sizes"][0] == 130 and (one["mode"] == 0).all()
    # three short trajectories 1 apart in one joint: a-b and b-c within 1.5, a-c not
    chain = np.zeros((3, 3, 4))
    chain[:, :, 0] = np.array([0.0, 1.0, 2.0])[:, None]
    for metric in METRICS:
        g = engine.group_traj(2, chain, [2.0, 1.0, 3.0], None, 1.5, None, metric)
        assert g["n_modes"] == 1 and list(g["mode"]) == [0, 0, 0] and list(g["leaders"]) == [1, -1, -1]
        g = engine.group_traj(2, chain, [1.0, 2.0, 3.0], None, 1.5, None, metric)
        assert g["n_modes"] == 2 and list(g["mode"]) == [0, 0, 1] and list(g["leaders"]) == [0, 2, -1] and list(g["sizes"]) == [2, 1, 0]
    g = engine.group_traj(2, chain, [1.0, 2.0, 3.0], [0, 0, 0], 1.5)
    assert g["n_modes"] == 0 and (g["mode"] == -1).all() and (g["leaders"] == -1).all()
    lib = engine.lib                                      # every output may be NULL; more rows than the limit
    assert lib.gpmp2mi_group_traj(2, 3, 2, E.dptr(chain), None, 0, 1.5, E.dptr(np.zeros(3)), None, None, None, None, None) == 0
    one_ = C.cast(C.c_void_p(1), E._capi.c_double_p)
    assert lib.gpmp2mi_group_traj(2, scoring.MAX_GROUP_ROWS + 1, 2, one_, None, 0, 1.5, one_, None, None, None, None, None) == 4
    assert b"8192" in lib.gpmp2mi_last_error()


_DEV = r"""
import numpy as np
import torch                      # torch's HIP runtime first, as bench.py does
torch.cuda.init()
import group_reference as gr
from gpmp2_amd import engine as E
eng = E.Engine()
rng = np.random.default_rng(3)
B, N, D = 130, 4, 7
traj, _ = gr.synthetic_modes(rng, 3, B, N, D)
score, eligible = gr.scores_with_ties(rng, B)
dev = lambda x, dt: torch.tensor(np.ascontiguousarray(x), dtype=dt, device="cuda")
t, sc, el = dev(traj, torch.float64), dev(score, torch.float64), dev(eligible, torch.int32)
st = torch.cuda.Stream()
w = np.linspace(0.0, 2.0, D)
for metric in (0, 1):
    for weights in (None, w):
        host = eng.traj_distances(D, traj, weights, metric)
        radius = gr.gap_radius(gr.distances(traj, D, weights, metric))
        dist = torch.full((B, B), float("nan"), dtype=torch.float64, device="cuda")
        outs = [torch.full((B,), 99, dtype=torch.int32, device="cuda") for _ in range(6)]
        n = torch.full((2,), 99, dtype=torch.int32, device="cuda")
        with torch.cuda.stream(st):
            eng.traj_distances_dev(D, B, N, t, dist, weights, metric, stream=st.cuda_stream)
            eng.group_rows_dev(B, dist, sc, el, radius, outs[0], outs[1], outs[2], n[0:1], stream=st.cuda_stream)
            eng.group_traj_dev(D, B, N, t, sc, el, radius, weights, metric, outs[3], outs[4], outs[5], n[1:2], stream=st.cuda_stream)
        st.synchronize()
        assert np.array_equal(dist.cpu().numpy().view(np.int64), host.view(np.int64)), "traj_distances_dev != traj_distances"
        want = eng.group_traj(D, traj, score, eligible, radius, weights, metric)
        for k, name in enumerate(("mode", "leaders", "sizes")):
            assert np.array_equal(outs[k].cpu().numpy(), want[name]), ("group_rows_dev", name)
            assert np.array_equal(outs[3 + k].cpu().numpy(), want[name]), ("group_traj_dev", name)
        assert n.cpu().tolist() == [want["n_modes"]] * 2
print("GROUP DEV OK")
"""


def test_dev_forms_equal_the_host_forms_next_to_torch():
    """fresh process: torch initialises the HIP runtime before the library, as bench.py does"""
    assert importlib.util.find_spec("torch") is not None    # not imported here: this process keeps the library's runtime
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")] +
                                                      [x for x in [os.environ.get("PYTHONPATH")] if x]))
    r = subprocess.run([sys.executable, "-c", _DEV], capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert r.returncode == 0 and "GROUP DEV OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ------------------------------------------------------------------------------------------------ plans
def _args(p):
    return p.start_conf, p.start_vel, p.end_conf, p.end_vel


def _solved(engine, p):
    r, s = engine.robot(p.model), engine.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)
    pl = engine.plan(r, s, p.setting, p.B)
    pl.set_problem(*_args(p), p.init)
    pl.optimize()
    return r, s, pl


@pytest.fixture(scope="module")
def wam8(engine):
    p = problems.wam_restarts(B=8, total_step=12, obs_check_inter=3, sdf="40")
    r, s, pl = _solved(engine, p)
    res = pl.result()
    dref = {m: gr.distances(res["traj"], 7, None, m) for m in METRICS}
    return dict(p=p, r=r, s=s, pl=pl, res=res, dref=dref, pairs=engine.generate_self_pairs(r, 2, np.zeros((1, 7))))


def _check_distinct(engine, pl, p, res, out, el, radius, metric, dref, J, lie, max_alt):
    D, fe = p.setting.dof, res["final_error"]
    g = engine.group_traj(D, res["traj"], fe, el.astype(np.int32), radius, None, metric)
    _same_groups(_as_dict(gr.rule(dref, fe, el, radius)), g, "group_traj vs reference")
    k = min(g["n_modes"], max_alt)
    assert out["n_modes"] == g["n_modes"] and np.array_equal(out["mode"], g["mode"])
    assert np.array_equal(out["alt"][:k], g["leaders"][:k]) and (out["alt"][k:] == -1).all()
    assert np.array_equal(out["alt_size"][:k], g["sizes"][:k]) and (out["alt_size"][k:] == 0).all()
    assert np.isnan(out["alt_error"][k:]).all() and np.isnan(out["traj_alt"][k:]).all() and np.isnan(out["dense_alt"][k:]).all()
    dt = ref.delta_t(p.setting)
    for j in range(k):
        row = int(out["alt"][j])
        assert out["alt_error"][j] == fe[row]
        assert np.array_equal(_bits(out["traj_alt"][j]), _bits(res["traj"][row]))
        up = engine.interpolate_traj(D, lie, None, dt, J, res["traj"][row][None])[0]
        if lie:
            np.testing.assert_allclose(out["dense_alt"][j], up, rtol=0, atol=1e-12)
        else:
            assert np.array_equal(_bits(out["dense_alt"][j]), _bits(up))
    return g


def test_plan_form_on_wam_restarts(engine, wam8):
    w = wam8
    p, pl, res, pairs = w["p"], w["pl"], w["res"], w["pairs"]
    J = 4
    sc, ss = pl.score(J), pl.self_score(pairs, J)
    for metric in METRICS:
        radius = gr.gap_radius(w["dref"][metric])
        for req, rir in ((-INF, False), (0.0, True)):
            sel = pl.select(J, req, rir)
            out = pl.select_distinct(J, radius, 8, req, rir, metric=metric)
            assert (int(out["alt"][0]), out["n_eligible"]) == (sel["best"], sel["n_eligible"])
            el = scoring.eligible(res["final_error"], res["status"], sc["min_clearance"], sc["out_of_range"], req, rir)
            g = _check_distinct(engine, pl, p, res, out, el, radius, metric, w["dref"][metric], J, False, 8)
            print(f"wam8 metric={metric} required_clearance={req}: {out['n_eligible']} eligible, {g['n_modes']} modes, "
                  f"sizes {list(g['sizes'][:g['n_modes']])}, radius {radius:.3e}")
            # with the self-collision rule
            for rsc in (0.0, -INF):
                chk = pl.select_checked(J, pairs, req, rir, rsc)
                out = pl.select_distinct(J, radius, 8, req, rir, pairs, rsc, metric=metric)
                assert (int(out["alt"][0]), out["n_eligible"]) == (chk["best"], chk["n_eligible"])
                el2 = scoring.eligible(res["final_error"], res["status"], sc["min_clearance"], sc["out_of_range"], req, rir,
                                       ss["min_self_clearance"], ss["invalid"], rsc)
                _check_distinct(engine, pl, p, res, out, el2, radius, metric, w["dref"][metric], J, False, 8)
    # max_alt = 1 with more than one mode: the full count, one entry; one mode of max_alt = 8: the other slabs stay
    dref = w["dref"][0]
    el = scoring.eligible(res["final_error"], res["status"], sc["min_clearance"], sc["out_of_range"], -INF, False)
    out = pl.select_distinct(J, 0.0, 1, -INF, False)
    assert out["n_modes"] == gr.rule(dref, res["final_error"], el, 0.0)[3] > 1 and out["alt"].shape == (1,)
    assert out["alt"][0] == pl.select(J, -INF, False)["best"] and out["traj_alt"].shape[0] == 1
    _check_distinct(engine, pl, p, res, out, el, 0.0, 0, dref, J, False, 1)
    out = pl.select_distinct(J, INF, 8, -INF, False)
    assert out["n_modes"] == 1 and out["alt_size"][0] == out["n_eligible"]
    _check_distinct(engine, pl, p, res, out, el, INF, 0, dref, J, False, 8)
    # weights: joint 0 alone
    wts = np.array([1.0, 0, 0, 0, 0, 0, 0])
    dw = gr.distances(res["traj"], 7, wts, 0)
    rw = gr.gap_radius(dw)
    out = pl.select_distinct(J, rw, 8, -INF, False, weights=wts)
    _same_groups(_as_dict(gr.rule(dw, res["final_error"], el, rw)),
                 engine.group_traj(7, res["traj"], res["final_error"], el.astype(np.int32), rw, wts), "weights")
    assert np.array_equal(out["mode"], gr.rule(dw, res["final_error"], el, rw)[0])


DEV_NAMES = ("n_modes", "n_eligible", "alt", "alt_size", "alt_error", "mode", "traj_alt", "dense_alt")


def _dev_outputs(engine, B, N, D, Md, max_alt):
    """the eight device outputs of select_distinct_dev, prefilled with 99 / NaN: what select_distinct(fill=nan) leaves
    in the entries it does not write, except alt / alt_size / n_modes / n_eligible, which are always written"""
    def ints(*shape):
        return _DevArray(engine, np.full(shape, 99, dtype=np.int32))

    def reals(*shape):
        return _DevArray(engine, np.full(shape, NAN))
    return dict(n_modes=ints(1), n_eligible=ints(1), alt=ints(max_alt), alt_size=ints(max_alt), alt_error=reals(max_alt),
                mode=ints(B), traj_alt=reals(max_alt, N + 1, 2 * D), dense_alt=reals(max_alt, Md, 2 * D))


def _same_as_host(dev, host, names=DEV_NAMES):
    """device outputs against the dict of select_distinct, bit for bit; outputs not in `names` still hold their prefill"""
    for k in DEV_NAMES:
        got = dev[k].read()
        if k not in names:
            untouched = np.full(got.shape, 99, dtype=np.int32) if got.dtype == np.int32 else np.full(got.shape, NAN)
            assert np.array_equal(got.view(np.int32), untouched.view(np.int32)), (k, "was written")
            continue
        want = np.asarray(host[k], dtype=got.dtype).reshape(got.shape)
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), (k, got, want)


def test_the_dev_form_writes_what_the_host_form_returns(engine, wam8):
    """select_distinct_dev with device outputs on the WAM plan: all outputs, some outputs, max_alt below and above
    n_modes, with and without the pair table; every output equals select_distinct bit for bit, the slabs and alt_error
    beyond n_modes keep their prefill, and an output that is not asked for is not written"""
    w = wam8
    p, pl, pairs = w["p"], w["pl"], w["pairs"]
    J, B, N, D = 4, p.B, p.setting.total_step, 7
    Md = scoring.checked_states(N, J)
    for metric in METRICS:
        radius = gr.gap_radius(w["dref"][metric])
        n_modes = pl.select_distinct(J, radius, 8, -INF, False, metric=metric)["n_modes"]
        assert 2 < n_modes < 8
        for max_alt, use_pairs, req in ((2, False, -INF), (8, False, -INF), (8, True, 0.0), (1, True, -INF)):
            kw = dict(required_clearance=req, require_in_range=True, pairs=pairs if use_pairs else None,
                      required_self_clearance=-INF, metric=metric)
            host = pl.select_distinct(J, radius, max_alt, **kw)
            dev = _dev_outputs(engine, B, N, D, Md, max_alt)
            pl.select_distinct_dev(J, radius, max_alt, **kw, **{k: v.ptr for k, v in dev.items()})
            _same_as_host(dev, host)
            for v in dev.values():
                v.free()
        # some outputs only: the others are left alone
        for names in (("n_modes", "mode"), ("alt", "traj_alt"), ("n_eligible", "alt_size", "alt_error", "dense_alt"), ()):
            host = pl.select_distinct(J, radius, 3, -INF, False, metric=metric)
            dev = _dev_outputs(engine, B, N, D, Md, 3)
            pl.select_distinct_dev(J, radius, 3, -INF, False, metric=metric, **{k: dev[k].ptr for k in names})
            _same_as_host(dev, host, names)
            for v in dev.values():
                v.free()
    # nothing eligible: the counts and alt / alt_size are written, the rest keeps its prefill
    host = pl.select_distinct(J, 1.0, 4, 1e9, False)
    dev = _dev_outputs(engine, B, N, D, Md, 4)
    pl.select_distinct_dev(J, 1.0, 4, 1e9, False, **{k: v.ptr for k, v in dev.items()})
    _same_as_host(dev, host)
    assert host["n_modes"] == 0 and (dev["alt"].read() == -1).all() and np.isnan(dev["traj_alt"].read()).all()
    for v in dev.values():
        v.free()


def test_select_distinct_dev_returns_while_its_stream_is_parked(engine, wam8):
    """the stream is parked by the stall hook: the call returns while it is (the outputs still hold their prefill), and
    after the release they hold what the host form returns.  One parked episode, bounded by the hook's max_ms."""
    import time
    w = wam8
    p, pl, lib = w["p"], w["pl"], engine.lib
    J, B, N, D, max_alt = 4, p.B, p.setting.total_step, 7, 8
    Md = scoring.checked_states(N, J)
    radius = gr.gap_radius(w["dref"][0])
    host = pl.select_distinct(J, radius, max_alt, 0.0, True)      # the plan's workspaces hold this shape from here on
    assert host["n_modes"] > 1
    dev = _dev_outputs(engine, B, N, D, Md, max_alt)
    st, tok = C.c_void_p(), C.c_void_p()
    engine._ck(lib.gpmp2mi_debug_stream_create(C.byref(st)))
    engine._ck(lib.gpmp2mi_debug_stall_begin(st, 3000, C.byref(tok)))     # parks the stream, 3 s at the most
    try:
        t0 = time.perf_counter()
        pl.select_distinct_dev(J, radius, max_alt, 0.0, True, stream=st.value, **{k: v.ptr for k, v in dev.items()})
        took = time.perf_counter() - t0
        parked = int(dev["n_modes"].read()[0]), int(dev["alt"].read()[0])   # the default stream does not wait for the parked one
    finally:
        engine._ck(lib.gpmp2mi_debug_stall_release(tok))          # releases the stall and waits for that stream
    assert took < 1.0 and parked == (99, 99), ("the call waited for its stream", took, parked)
    _same_as_host(dev, host)
    for v in dev.values():
        v.free()


def test_plan_form_on_a_pose2_robot(engine):
    """config 5 is one row: no pair, so any radius satisfies the gap condition; dense_alt goes through the Pose2
    interpolator, equal to gpmp2mi_interpolate_traj within the 1e-12 the header states for dense_best"""
    p = problems.mobile_arm_config5()
    r, s, pl = _solved(engine, p)
    res = pl.result()
    for metric in METRICS:
        for J in (0, 3):
            sel = pl.select(J, -INF, False)
            out = pl.select_distinct(J, 1.0, 4, -INF, False, metric=metric)
            assert (int(out["alt"][0]), out["n_eligible"], out["n_modes"]) == (sel["best"], sel["n_eligible"], 1) == (0, 1, 1)
            _check_distinct(engine, pl, p, res, out, np.ones(1, dtype=bool), 1.0, metric, gr.distances(res["traj"], 5, None, metric),
                            J, True, 4)
            print(f"config5 metric={metric} inter_step={J}: dense_alt[0] bitwise dense_best of select "
                  f"{np.array_equal(_bits(out['dense_alt'][0]), _bits(sel['dense_best']))}")
    none = pl.select_distinct(2, 1.0, 4, 1e9, False)       # nothing eligible
    assert none["n_modes"] == 0 and none["n_eligible"] == 0 and (none["alt"] == -1).all() and (none["mode"] == -1).all()
    assert np.isnan(none["traj_alt"]).all()
    pl.close()


def test_the_optimizer_state_is_left_alone(engine, wam8):
    p, r, s, pairs = wam8["p"], wam8["r"], wam8["s"], wam8["pairs"]
    plans = []
    for with_call in (False, True):
        pl = engine.plan(r, s, p.setting, p.B)
        pl.set_problem(*_args(p), p.init)
        pl.optimize()
        if with_call:
            before = pl.select(4, 0.0, True)
            pl.select_distinct(4, 0.5, 8, 0.0, True)
            pl.select_distinct(2, 0.5, 3, 0.0, True, pairs, 0.0, metric=1)
            after = pl.select(4, 0.0, True)
            assert (before["best"], before["n_eligible"]) == (after["best"], after["n_eligible"])
        pl.update(1)
        plans.append((pl, pl.result()))
    for k in ("traj", "final_error", "iters", "status"):
        assert np.array_equal(plans[0][1][k], plans[1][1][k]), k
    for pl, _ in plans:
        pl.close()


def test_plan_states_and_arguments(engine, wam8):
    p, r, s = wam8["p"], wam8["r"], wam8["s"]
    pl = engine.plan(r, s, p.setting, p.B)
    with pytest.raises(E.Gpmp2miError) as ei:
        pl.select_distinct(2, 1.0)                         # nothing to group yet
    assert ei.value.code == 1 and "not been optimized" in str(ei.value)
    pl.set_problem(*_args(p), p.init)
    pl.optimize()
    lib, n = engine.lib, C.c_int(7)
    bad = [dict(inter=-1), dict(metric=2), dict(radius=-1.0), dict(radius=NAN), dict(max_alt=0), dict(max_alt=65),
           dict(weights=E.dptr(np.array([1.0, 1, 1, 1, 1, 1, -1])))]
    for kw in bad:
        a = dict(inter=2, metric=0, radius=1.0, max_alt=4, weights=None)
        a.update(kw)
        assert lib.gpmp2mi_plan_select_distinct(pl.h.ptr, a["inter"], 0.0, 0, None, 0.0, a["metric"], a["weights"], a["radius"],
                                                a["max_alt"], C.byref(n), None, None, None, None, None, None, None) == 1, kw
        assert n.value == 7
    assert lib.gpmp2mi_plan_select_distinct(pl.h.ptr, 2, 0.0, 0, None, 0.0, 0, None, 1.0, 4, None, None, None, None, None, None,
                                            None, None) == 0   # every output may be NULL
    pl.optimize_queue(*_args(p), p.init)                   # a queue run leaves no problem behind
    with pytest.raises(E.Gpmp2miError) as ei:
        pl.select_distinct(2, 1.0)
    assert ei.value.code == 1
    pl.close()
