// Builds against include/gpmp2mi_planner.hpp with plain g++ and links the product library.  The selection overload that
// takes the results re-timed under torque limits is host code and runs everywhere; the profile needs the GPU: without one
// it must throw (no silent fallback), with one the planar two-link arm at rest runs at max_rate under the torques of its
// textbook closed form, a constant-velocity line keeps every torque within its limit and is never slower than the
// uniform stretch, a handle without limits gives the profile of RetimeTrajectory bit for bit, and weak drives are STATIC.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>

#include "gpmp2mi_planner.hpp"

using namespace gpmp2mi;

static TrajectoryScore score(double clearance, int out_of_range) {
  TrajectoryScore s;
  s.min_clearance = clearance;
  s.out_of_range = out_of_range;
  return s;
}
static TrajectoryMotionScore motion(double pos_margin, int invalid) {
  TrajectoryMotionScore s;
  s.pos_margin = pos_margin;
  s.invalid = invalid;
  return s;
}
static DynamicRetimedTrajectory retimed(int status, double duration, double coef = 0.0) {
  DynamicRetimedTrajectory r;
  r.status = status;
  r.duration = duration;
  r.coef = {1.0, coef, 2.0};
  return r;
}

int main() {
  try {
    // the rule alone: row 1 is the cheapest but gravity alone is too much, row 2 has a non-finite quantity, row 3 takes
    // too long, row 4 re-times but one of its coefficients is not finite
    const double inf = std::numeric_limits<double>::infinity();
    const Vector fe{5.0, 1.0, 2.0, 3.0, 4.0, 0.5};
    const std::vector<int> status{0, 0, 0, 0, 0, GPMP2MI_TRAJ_NOT_SPD};
    const std::vector<TrajectoryScore> sc{score(0.1, 0), score(0.1, 0), score(0.1, 0), score(0.05, 0), score(0.2, 0), score(0.3, 0)};
    const std::vector<TrajectoryMotionScore> ms{motion(0.3, 0), motion(0.2, 0), motion(0.5, 2), motion(0.2, 0), motion(0.01, 0),
                                                motion(0.3, 0)};
    const std::vector<DynamicRetimedTrajectory> rt{retimed(GPMP2MI_RETIME_OK, 1.9), retimed(GPMP2MI_RETIME_STATIC, inf),
                                                   retimed(GPMP2MI_RETIME_OK, 1.5), retimed(GPMP2MI_RETIME_OK, 3.5),
                                                   retimed(GPMP2MI_RETIME_OK, 1.0, inf), retimed(GPMP2MI_RETIME_OK, 0.4)};
    std::size_t n = 99;
    if (SelectBestTrajectory(fe, status, sc, ms, rt, 0.0, 2.0, 0.0, false, &n) != 0 || n != 1) return 11;
    if (SelectBestTrajectory(fe, status, sc, ms, rt, 0.0, inf, 0.0, false, &n) != 3 || n != 2) return 12;
    if (SelectBestTrajectory(fe, status, sc, ms, rt, 0.25, inf, 0.0, false, &n) != 0 || n != 1) return 13;
    if (SelectBestTrajectory(fe, status, sc, ms, rt, 0.0, 1.0, 0.0, false, &n) != -1 || n != 0) return 14;
    bool threw = false;
    try {
      SelectBestTrajectory(fe, status, sc, ms, rt, 0.0, std::nan(""));
    } catch (const std::runtime_error&) {
      threw = true;
    }
    if (!threw) return 15;
    std::printf("SELECT OK\n");

    // the planar two-link arm in the world's x-y plane, gravity along -y, the centres of mass on the links' x axes
    const double l1 = 0.5, m1 = 1.3, m2 = 0.9, lc1 = l1 - 0.22, lc2 = 0.5 - 0.27, g = 9.81;
    Arm arm(2, {0.5, 0.5}, {0.0, 0.0}, {0.0, 0.0}, Pose3::Translation(0.0, 0.0, 0.0));
    BodySphereVector spheres;
    for (int l = 0; l < 2; l++) spheres.emplace_back(l, 0.05, std::array<double, 3>{-0.25, 0.0, 0.0});
    ArmModel model(arm, spheres);
    const Vector mass{m1, m2}, com{-0.22, 0.0, 0.0, -0.27, 0.0, 0.0};
    const Vector inertia{0.002, 0.03, 0.031, 0.0, 0.0, 0.0, 0.001, 0.02, 0.0205, 0.0, 0.0, 0.0};
    ArmDynamics dyn(model, mass, com, inertia, {14.0, 4.0}, {0.0, -g, 0.0});
    MotionLimits limits;
    limits.vel = {1.0, 1.0};
    TrajOptimizerSetting setting(2);
    setting.set_total_step(8);
    setting.set_total_time(2.0);
    const std::size_t J = 3, Md = 8 * (J + 1) + 1;
    // at rest, stretched out along x: nothing but gravity, and nothing to slow down for
    Trajectory rest = initArmTrajStraightLine({0.0, 0.0}, {0.0, 0.0}, 8);
    const DynamicRetimedTrajectory r = RetimeTrajectory(model, dyn, limits, rest, setting, J, 2.0);
    const double g1 = (m1 * lc1 + m2 * l1) * g + m2 * lc2 * g, g2 = m2 * lc2 * g;
    std::printf("REST status=%d duration=%.9f sdot=%.3f tau=%.9f %.9f achieved=%.9f %.9f\n", r.status, r.duration, r.sdot[0],
                r.tau[0], r.tau[1], r.achieved[4], r.achieved[5]);
    if (r.status != GPMP2MI_RETIME_OK || r.tau.size() != Md * 2 || r.coef.size() != Md * 8 || r.sdot.size() != Md) return 21;
    if (std::fabs(r.tau[0] - g1) > 1e-12 || std::fabs(r.tau[1] - g2) > 1e-12) return 22;
    if (r.sdot[Md / 2] != 2.0 || std::fabs(r.duration - 1.0) > 1e-12) return 23;
    if (r.achieved[4] != r.achieved[5] || std::fabs(r.achieved[5] - g1 / 14.0) > 1e-12) return 24;
    if (r.coef[0] != 0.0 || r.coef[1] != 0.0) return 25;   // p == 0 exactly where q' == 0
    // joint 0 at a constant 0.7 rad/s, the elbow bent by 0.5
    Trajectory line = initArmTrajStraightLine({-0.2, 0.5}, {1.2, 0.5}, 8);
    for (std::size_t i = 0; i <= 8; i++) {
      line.data[i * 4 + 2] = 0.7;
      line.data[i * 4 + 3] = 0.0;
    }
    const TrajectoryTorqueScore ts = TorqueScore(model, dyn, line, setting, J);
    const DynamicRetimedTrajectory t = RetimeTrajectory(model, dyn, limits, line, setting, J, 2.0);
    const double stretch = std::fmax(std::fmax(ts.time_scale, 0.7), 0.5) * 2.0;
    std::printf("LINE status=%d uniform=%.6f retimed=%.6f achieved=%.9f %.9f %.9f\n", t.status, stretch, t.duration,
                t.achieved[0], t.achieved[4], t.achieved[5]);
    if (t.status != GPMP2MI_RETIME_OK || !(t.duration <= stretch * (1.0 + 1e-12)) || !(t.duration >= 1.0 - 1e-12)) return 31;
    if (!(t.achieved[4] <= 1.0 + 1e-12) || !(t.achieved[0] <= 1.0 + 1e-9) || !(t.achieved[5] < 1.0)) return 32;
    if (std::fabs(t.achieved[5] - ts.static_ratio) > 1e-12) return 33;
    const std::size_t k = Md / 2;   // the torque at planned timing is m + tau_g
    for (std::size_t d = 0; d < 2; d++)
      if (std::fabs(t.coef[k * 8 + 4 + d] + t.coef[k * 8 + 6 + d] - ts.tau[2 * k + d]) > 1e-9) return 34;
    for (std::size_t i = 0; i < Md; i++) {   // the torques of the re-timed result are its rows
      const std::size_t s = i + 1 < Md ? i : i - 1;
      for (std::size_t d = 0; d < 2; d++) {
        const double m = t.coef[i * 8 + (i + 1 < Md ? 4 : 2) + d], p = t.coef[i * 8 + d], tg = t.coef[i * 8 + 6 + d];
        if (std::fabs(t.tau[2 * i + d] - (m * t.sdot[i] * t.sdot[i] + p * t.u[s] + tg)) > 1e-9) return 35;
      }
    }
    // a handle without limits: the profile of RetimeTrajectory, bit for bit
    ArmDynamics none(model, mass, com, inertia, {}, {0.0, -g, 0.0});
    const DynamicRetimedTrajectory f = RetimeTrajectory(model, none, limits, line, setting, J, 2.0);
    const RetimedTrajectory plain = RetimeTrajectory(model, limits, line, setting, J, 2.0);
    if (f.status != plain.status || std::memcmp(&f.duration, &plain.duration, sizeof(double)) != 0 ||
        std::memcmp(f.sdot.data(), plain.sdot.data(), Md * sizeof(double)) != 0 ||
        std::memcmp(f.stamps.data(), plain.stamps.data(), Md * sizeof(double)) != 0 || f.achieved[4] != 0.0)
      return 41;
    if (!(t.duration >= plain.duration)) return 42;
    // weak drives: gravity alone is too much, no timing helps, and the selection never takes such a result
    ArmDynamics weak(model, mass, com, inertia, {1.0, 1.0}, {0.0, -g, 0.0});
    const DynamicRetimedTrajectory w = RetimeTrajectory(model, weak, limits, line, setting, J, 2.0);
    if (w.status != GPMP2MI_RETIME_STATIC || w.duration != inf || w.sdot[0] == w.sdot[0] || w.tau[0] == w.tau[0]) return 43;
    const std::vector<TrajectoryScore> clear{score(0.5, 0), score(0.5, 0)};
    const std::vector<TrajectoryMotionScore> free{motion(inf, 0), motion(inf, 0)};
    const int best = SelectBestTrajectory({2.0, 1.0}, {}, clear, free, {t, w}, -inf, inf, 0.0, false, &n);
    if (best != 0 || n != 1) return 44;
    std::printf("OK best=%d of %zu eligible\n", best, n);
    return 0;
  } catch (const std::exception& e) {
    std::printf("EXCEPTION %s\n", e.what());
    return 3;
  }
}
