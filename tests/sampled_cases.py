"""The cases the sampled-clearance tests share (tests/test_sampled_cpu.py pins their thresholds on the CPU,
tests/test_gpu_sampled.py runs them on the device): three robots at six (N, J), every row at one seed.

    planar  the two-link arm of tests/test_cpp_risk.py on its planar field, 4 spheres
    point   a point robot on the planar field of problems.point_robot_2d
    wam     the WAM on the down-scaled desk scene, 16 spheres

    arm3, arm5, arm6   planar arms of 3, 5 and 6 joints at (21, 2): the other widths of the bridge normals

(N, J): (1, 0) two checked states, (1, 5) one interval, (5, 5), (16, 3) with Md = 65 and (33, 1) with Md = 67 -- one and
three states past a tile, the second with an interval across the tile border (the halo) -- and (2, 63), the largest J.
At N = 1 row 2 of the planar arm and of the point robot nearly rests at a clearance of 0.08, and the point robot at (5, 5)
has a seed of its own: the conditions of tests/test_sampled_cpu.py on the thresholds asked for that.
Every case is evaluated at its initial values: the estimate is p.init, the precision the oracle's linearization there.
"""
from __future__ import annotations

import numpy as np

import sampled_reference as ref
import score_reference as sref
from gpmp2_amd import problems

NJ = ((1, 0), (1, 5), (5, 5), (16, 3), (33, 1), (2, 63))
ROBOTS = ("planar", "point", "wam")
SEED = 20261018
SEEDS = {("point", 5, 5): 16}                 # (robot, N, J) -> the seed of a case that needs another one (tests/test_sampled_cpu.py says why)
K_REF = 17                 # the reference is made once for 17 samples; K = 1 and 16 are its prefixes
KS = (1, 16, 17)
ROW_FIRST, SAMPLE_FIRST = 5, 3
B = 3


def _args(p):
    return p.start_conf, p.start_vel, p.end_conf, p.end_vel


def _line(start, end, N, total_time):
    init = np.zeros((B, N + 1, 2 * start.shape[1]))
    D = start.shape[1]
    for b in range(B):
        for i in range(N + 1):
            init[b, i, :D] = start[b] * (N - i) / N + end[b] * i / N
        init[b, :, D:] = (end[b] - start[b]) / total_time
    return init


def planar(N):
    import gpmp2_amd as g
    arm = g.Arm(2, [1.0, 1.0], [0.0, 0.0], [0.0, 0.0])
    model = g.ArmModel(arm, [g.BodySphere(l, 0.1, (x, 0.0, 0.0)) for l in range(2) for x in (-0.75, -0.25)])
    cells = 60
    x, y = np.meshgrid(np.arange(cells), np.arange(cells))      # field[y][x]
    field = np.hypot(-3.0 + 0.1 * x - 1.2, -3.0 + 0.1 * y - 1.0) - 0.4
    st = g.TrajOptimizerSetting(2)
    T = 0.2 * N
    st.set_total_step(N); st.set_total_time(T); st.set_obs_check_inter(2); st.set_cost_sigma(0.1); st.set_epsilon(0.2)
    st.set_Qc_model(np.array([[1.0, 0.3], [0.3, 0.5]]))
    st.setGaussNewton()
    start = np.zeros((B, 2))
    end = np.array([[1.5, 0.5], [1.2, 0.9], [0.4, -0.6]])
    if N == 1:      # one interval: row 2 nearly rests where its clearance is 0.08, so that the sub-steps straddle T_map
        start[2], end[2] = [0.9825, 0.3], [0.9845, 0.3]
    z = np.zeros((B, 2))
    return problems.Problem("planar two-link arm", model, [-3.0, -3.0], 0.1, field, st, start, z, end, z.copy(),
                            _line(start, end, N, T))


def point(N):
    p = problems.point_robot_2d()
    st = p.setting
    T = 0.5 * N
    st.set_total_step(N); st.set_total_time(T)
    start = np.tile(p.start_conf, (B, 1))
    end = p.end_conf + np.array([[0.0, 0.0], [-4.0, 1.5], [1.0, -6.0]])
    if N == 1:      # as the planar arm: row 2 nearly rests at a clearance of 0.08
        start[2], end[2] = [-6.5, -8.0], [-6.495, -8.0]
    z = np.zeros((B, 2))
    return problems.Problem("point robot, three goals", p.model, p.sdf_origin, p.sdf_cell, p.sdf_data, st, start, z, end,
                            z.copy(), _line(start, end, N, T))


def wam(N):
    return problems.wam_restarts(B=B, total_step=N, obs_check_inter=2, opt="GN", sdf="40")


def arm(D):
    """the planar arm of D joints of tests/test_gpu_step_backward_error.py (N = 21, one sphere a link): the widths of the
    pairing of the bridge normals that the three robots above do not reach (D = 3: sine members unused; 5, 6: some used)"""
    def make(N):
        from test_gpu_step_backward_error import _planar
        p = _planar(D)
        assert p.setting.total_step == N
        return p
    return make


MAKE = dict(planar=planar, point=point, wam=wam, arm3=arm(3), arm5=arm(5), arm6=arm(6))
EXTRA = (("arm3", 21, 2), ("arm5", 21, 2), ("arm6", 21, 2))
ALL = tuple((r, N, J) for r in ROBOTS for N, J in NJ) + EXTRA
_CTX = {}


class Ctx:
    """a case with the oracle's handles, its linearization at the initial values and the float64 support samples"""

    def __init__(self, oracle, robot, N, J):
        p = MAKE[robot](N)
        self.p, self.robot, self.N, self.J, self.D = p, robot, N, J, p.setting.dof
        self.dt, self.Qc = sref.delta_t(p.setting), p.setting.Qc
        self.oracle, self.ro = oracle, oracle.robot(p.model)
        self.fld = sref.oracle_sdf(oracle, p.sdf_origin, p.sdf_cell, p.sdf_data)
        self.radius = np.asarray(p.model.flat()["sphere_radius"], dtype=np.float64)
        self.seed = SEEDS.get((robot, N, J), SEED)
        self.est = np.ascontiguousarray(p.init)
        self.Hd, self.Ho, _, _ = oracle.linearize(self.ro, self.fld.handle, p.setting, *_args(p), self.est)
        self.delta = np.stack([ref.support_samples(self.Hd[b], self.Ho[b], self.seed, ROW_FIRST + b, SAMPLE_FIRST, K_REF)
                               for b in range(B)])
        self._rows = {}

    def row(self, b, bridge, delta=None, Lp=None):
        """the reference of row b for the K_REF samples (cached for the float64 samples and the long-double factor)"""
        key = (b, bool(bridge))
        if delta is None and Lp is None:
            if key not in self._rows:
                self._rows[key] = self.row(b, bridge, self.delta[b])
            return self._rows[key]
        d = self.delta[b] if delta is None else delta
        return ref.row(self.oracle, self.ro, self.fld, self.radius, self.Qc, self.D, self.dt, self.J, self.est[b], d,
                       self.seed, ROW_FIRST + b, SAMPLE_FIRST, bridge, Lp)

    def spread(self, b, bridge):
        """e_cpu of row b: the reference on float64 support samples against the same on long-double ones, on both maps as
        float64 holds them (the device answers in float64: a spread below its resolution is none)"""
        dl = ref.support_samples(self.Hd[b], self.Ho[b], self.seed, ROW_FIRST + b, SAMPLE_FIRST, K_REF, ref.LD)
        a, c = self.row(b, bridge), self.row(b, bridge, dl)
        fin = np.isfinite(a["state"]) & np.isfinite(c["state"])
        return (float(np.abs(a["conf"].astype(np.float64) - c["conf"].astype(np.float64)).max()),
                float(np.abs(a["state"][fin] - c["state"][fin]).max()) if fin.any() else 0.0)


def ctx(oracle, robot, N, J):
    if (robot, N, J) not in _CTX:
        _CTX[(robot, N, J)] = Ctx(oracle, robot, N, J)
    return _CTX[(robot, N, J)]
