// Builds against include/gpmp2mi_planner.hpp with plain g++ and links the product library.  The selection overload that
// takes the torque scores is host code and runs everywhere; the torques need the GPU: without one the call must throw (no
// silent fallback), with one the planar two-link arm at rest and on a constant-velocity line gives the torques of its
// textbook closed form.
#include <cmath>
#include <cstdio>
#include <limits>

#include "gpmp2mi_planner.hpp"

using namespace gpmp2mi;

static TrajectoryScore score(double clearance, int out_of_range) {
  TrajectoryScore s;
  s.min_clearance = clearance;
  s.out_of_range = out_of_range;
  return s;
}
static TrajectoryMotionScore motion(double pos_margin, double time_scale, int invalid) {
  TrajectoryMotionScore s;
  s.pos_margin = pos_margin;
  s.time_scale = time_scale;
  s.invalid = invalid;
  return s;
}
static TrajectoryTorqueScore torque(double time_scale, int invalid) {
  TrajectoryTorqueScore s;
  s.time_scale = time_scale;
  s.invalid = invalid;
  return s;
}

int main() {
  try {
    // the rule alone: row 1 is the cheapest but its drives need the larger stretch, row 2 has a non-finite torque, row 3
    // is held up by gravity alone
    const double inf = std::numeric_limits<double>::infinity();
    const Vector fe{5.0, 1.0, 2.0, 3.0, 4.0, 0.5};
    const std::vector<int> status{0, 0, 0, 0, 1, GPMP2MI_TRAJ_NOT_SPD};
    const std::vector<TrajectoryScore> sc{score(0.1, 0), score(0.1, 0), score(0.1, 0), score(0.05, 0), score(0.2, 3), score(0.3, 0)};
    const std::vector<TrajectoryMotionScore> ms{motion(0.3, 0.9, 0), motion(0.2, 0.5, 0), motion(0.5, 0.5, 0), motion(0.2, 0.5, 0),
                                                motion(0.01, 1.2, 0), motion(0.3, 0.1, 0)};
    const std::vector<TrajectoryTorqueScore> ts{torque(0.5, 0), torque(1.8, 0), torque(0.2, 3), torque(inf, 0), torque(0.4, 0),
                                                torque(0.1, 0)};
    std::size_t n = 99;
    if (SelectBestTrajectory(fe, status, sc, ms, ts, 0.0, 1.5, 0.0, false, &n) != 4 || n != 2) return 11;
    if (SelectBestTrajectory(fe, status, sc, ms, ts, 0.0, 1.5, 0.0, true, &n) != 0 || n != 1) return 12;
    if (SelectBestTrajectory(fe, status, sc, ms, ts, 0.0, 1.8, 0.0, false, &n) != 1 || n != 3) return 13;
    if (SelectBestTrajectory(fe, status, sc, ms, ts, 0.0, 1.0, 0.0, false, &n) != 0 || n != 1) return 14;
    if (SelectBestTrajectory(fe, status, sc, ms, ts, 0.0, 0.8, 0.0, false, &n) != -1 || n != 0) return 15;
    if (SelectBestTrajectory(fe, status, sc, ms, ts, 0.25, 1e300, 0.0, false, &n) != 0 || n != 1) return 16;
    bool threw = false;
    try {
      SelectBestTrajectory(fe, status, sc, ms, ts, 0.0, std::nan(""));
    } catch (const std::runtime_error&) {
      threw = true;
    }
    if (!threw) return 17;
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
    TrajOptimizerSetting setting(2);
    setting.set_total_step(8);
    setting.set_total_time(2.0);
    const std::size_t J = 3, Md = 8 * (J + 1) + 1;
    // at rest, stretched out along x: gravity alone
    Trajectory rest = initArmTrajStraightLine({0.0, 0.0}, {0.0, 0.0}, 8);
    const TrajectoryTorqueScore r = TorqueScore(model, dyn, rest, setting, J);
    const double g1 = (m1 * lc1 + m2 * l1) * g + m2 * lc2 * g, g2 = m2 * lc2 * g;
    std::printf("REST ratio=%.9f static=%.9f scale=%.3g tau=%.9f %.9f\n", r.torque_ratio, r.static_ratio, r.time_scale, r.tau[0],
                r.tau[1]);
    if (r.tau.size() != Md * 2 || r.invalid != 0) return 21;
    if (std::fabs(r.tau[0] - g1) > 1e-12 || std::fabs(r.tau[1] - g2) > 1e-12) return 22;
    if (r.torque_ratio != r.static_ratio || r.time_scale != 0.0 || std::fabs(r.static_ratio - g1 / 14.0) > 1e-12) return 23;
    if (r.static_joint != 0 || r.torque_joint != 0) return 24;
    // joint 0 at a constant 0.7 rad/s, the elbow bent by 0.5: the elbow feels the centripetal term m2 l1 lc2 sin(q2) q1'^2
    Trajectory line = initArmTrajStraightLine({-0.2, 0.5}, {1.2, 0.5}, 8);
    for (std::size_t i = 0; i <= 8; i++) {
      line.data[i * 4 + 2] = 0.7;
      line.data[i * 4 + 3] = 0.0;
    }
    const TrajectoryTorqueScore t = TorqueScore(model, dyn, line, setting, J);
    const std::size_t k = Md / 2;
    const double q1 = -0.2 + 1.4 * static_cast<double>(k) / static_cast<double>(Md - 1), q2 = 0.5;
    const double e2 = m2 * l1 * lc2 * std::sin(q2) * 0.49 + m2 * lc2 * g * std::cos(q1 + q2);
    const double e1 = (m1 * lc1 + m2 * l1) * g * std::cos(q1) + m2 * lc2 * g * std::cos(q1 + q2);
    std::printf("LINE ratio=%.6f static=%.6f scale=%.6f tau=%.9f %.9f want %.9f %.9f\n", t.torque_ratio, t.static_ratio,
                t.time_scale, t.tau[2 * k], t.tau[2 * k + 1], e1, e2);
    if (std::fabs(t.tau[2 * k] - e1) > 1e-9 || std::fabs(t.tau[2 * k + 1] - e2) > 1e-9) return 31;
    if (!(t.static_ratio < 1.0) || !((t.torque_ratio <= 1.0) == (t.time_scale <= 1.0)) || !(t.time_scale > 0.0)) return 32;
    // a handle with weak drives: gravity alone is too much, and the selection never takes such a row
    ArmDynamics weak(model, mass, com, inertia, {1.0, 1.0}, {0.0, -g, 0.0});
    const TrajectoryTorqueScore w = TorqueScore(model, weak, line, setting, J);
    if (!(w.static_ratio >= 1.0) || w.time_scale != inf) return 33;
    const std::vector<TrajectoryScore> clear{score(0.5, 0), score(0.5, 0)};
    const std::vector<TrajectoryMotionScore> free{motion(inf, 0.0, 0), motion(inf, 0.0, 0)};
    const int best = SelectBestTrajectory({2.0, 1.0}, {}, clear, free, {t, w}, -inf, inf, 0.0, false, &n);
    if (best != 1 || n != 2) return 34;          // +inf <= +inf: no bound was asked for
    const int bounded = SelectBestTrajectory({2.0, 1.0}, {}, clear, free, {t, w}, -inf, 1e6, 0.0, false, &n);
    if (bounded != 0 || n != 1) return 35;
    std::printf("OK best=%d of %zu eligible\n", bounded, n);
    return 0;
  } catch (const std::exception& e) {
    std::printf("EXCEPTION %s\n", e.what());
    return 3;
  }
}
