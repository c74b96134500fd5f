// Builds against include/gpmp2mi_planner.hpp with plain g++ and links the product library.  The selection overload that
// takes the re-timed results is host code and runs everywhere; the profile needs the GPU: without one it must throw (no
// silent fallback), with one a 3-link arm on a constant-velocity line runs at its cap throughout, and a line with one
// fast support state is slowed around that state only.
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
static TrajectoryMotionScore motion(double pos_margin, int invalid) {
  TrajectoryMotionScore s;
  s.pos_margin = pos_margin;
  s.invalid = invalid;
  return s;
}
static RetimedTrajectory retimed(int status, double duration) {
  RetimedTrajectory r;
  r.status = status;
  r.duration = duration;
  return r;
}

int main() {
  try {
    // the rule alone: row 1 is the cheapest but does not re-time, row 2 has a non-finite quantity, row 3 takes too long
    const double inf = std::numeric_limits<double>::infinity();
    const Vector fe{5.0, 1.0, 2.0, 3.0, 4.0, 0.5};
    const std::vector<int> status{0, 0, 0, 0, 1, GPMP2MI_TRAJ_NOT_SPD};
    const std::vector<TrajectoryScore> sc{score(0.1, 0), score(0.1, 0), score(0.1, 0), score(0.05, 0), score(0.2, 3), score(0.3, 0)};
    const std::vector<TrajectoryMotionScore> ms{motion(0.3, 0), motion(0.2, 0), motion(0.5, 2), motion(0.2, 0), motion(0.01, 0),
                                                motion(0.3, 0)};
    const std::vector<RetimedTrajectory> rt{retimed(GPMP2MI_RETIME_OK, 1.9), retimed(GPMP2MI_RETIME_EMPTY, inf),
                                            retimed(GPMP2MI_RETIME_OK, 1.5), retimed(GPMP2MI_RETIME_OK, 3.5),
                                            retimed(GPMP2MI_RETIME_OK, 2.0), retimed(GPMP2MI_RETIME_OK, 0.4)};
    std::size_t n = 99;
    if (SelectBestTrajectory(fe, status, sc, ms, rt, 0.0, 2.0, 0.0, false, &n) != 4 || n != 2) return 11;
    if (SelectBestTrajectory(fe, status, sc, ms, rt, 0.0, 2.0, 0.0, true, &n) != 0 || n != 1) return 12;
    if (SelectBestTrajectory(fe, status, sc, ms, rt, 0.0, inf, 0.0, false, &n) != 3 || n != 3) return 13;
    if (SelectBestTrajectory(fe, status, sc, ms, rt, 0.25, inf, 0.0, false, &n) != 0 || n != 1) return 14;
    if (SelectBestTrajectory(fe, status, sc, ms, rt, 0.0, 1.0, 0.0, false, &n) != -1 || n != 0) return 15;
    bool threw = false;
    try {
      SelectBestTrajectory(fe, status, sc, ms, rt, 0.0, std::nan(""));
    } catch (const std::runtime_error&) {
      threw = true;
    }
    if (!threw) return 16;
    std::printf("SELECT OK\n");

    Arm arm(3, {0.5, 0.5, 0.5}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, Pose3::Translation(0.0, 0.0, 0.0));
    BodySphereVector spheres;
    for (int l = 0; l < 3; l++)
      for (double x : {-0.375, -0.125}) spheres.emplace_back(l, 0.06, std::array<double, 3>{x, 0.0, 0.0});
    ArmModel model(arm, spheres);
    MotionLimits limits;
    limits.vel = {1.0, 1.0, 1.0};
    limits.acc = {4.0, 4.0, 4.0};
    limits.point_speed = 1.0;
    TrajOptimizerSetting setting(3);
    setting.set_total_step(8);
    setting.set_total_time(2.0);
    const std::size_t J = 4, Md = 8 * (J + 1) + 1;
    // a constant-velocity line in joint 0: 0.7 rad/s, the outermost sphere just under the Cartesian limit
    Trajectory line = initArmTrajStraightLine({-0.2, 0.1, -0.1}, {1.2, 0.1, -0.1}, 8);
    for (std::size_t i = 0; i <= 8; i++)
      for (std::size_t d = 0; d < 3; d++) line.data[i * 6 + 3 + d] = (line.data[8 * 6 + d] - line.data[d]) / 2.0;
    const TrajectoryMotionScore lm = MotionScoreTrajectory(model, limits, line, setting, J);
    const RetimedTrajectory lr = RetimeTrajectory(model, limits, line, setting, J, 2.0);
    std::printf("LINE scale=%.6f duration=%.6f sdot=%.6f achieved=%.6f %.6f %.6f %.6f\n", lm.time_scale, lr.duration, lr.sdot[0],
                lr.achieved[0], lr.achieved[1], lr.achieved[2], lr.achieved[3]);
    if (lr.status != GPMP2MI_RETIME_OK || lr.sdot.size() != Md || lr.dense.total_step + 1 != Md) return 21;
    // nothing accelerates, the cap is the same at every state: the whole row runs at 1 / time_scale
    if (std::fabs(lr.duration - 2.0 * lm.time_scale) > 1e-12 || std::fabs(lr.sdot[Md / 2] * lm.time_scale - 1.0) > 1e-12) return 22;
    if (std::fabs(lr.achieved[3] - 1.0) > 1e-12 || !(lr.achieved[1] < 1e-9) || std::fabs(lr.stamps[Md - 1] - lr.duration) != 0.0) return 23;
    if (std::fabs(lr.dense.v(0)[0] - 0.7 * lr.sdot[0]) > 1e-12) return 24;
    // the same line with one support state three times too fast in joint 1: the uniform stretch slows all of it
    Trajectory corner = line;
    corner.v(4)[1] = 3.0;
    const TrajectoryMotionScore cm = MotionScoreTrajectory(model, limits, corner, setting, J);
    const RetimedTrajectory cr = RetimeTrajectory(model, limits, corner, setting, J, 2.0);
    const RetimedTrajectory slow = RetimeTrajectory(model, limits, corner, setting, J, 1.0);
    const RetimedTrajectory rest = RetimeTrajectory(model, limits, corner, setting, J, 2.0, 0.0, 0.0);
    std::printf("CORNER uniform=%.4f retimed=%.4f as-planned-or-slower=%.4f from-rest=%.4f achieved=%.6f %.6f %.6f %.6f\n",
                cm.time_scale * 2.0, cr.duration, slow.duration, rest.duration, cr.achieved[0], cr.achieved[1], cr.achieved[2],
                cr.achieved[3]);
    if (cr.status != GPMP2MI_RETIME_OK || slow.status != GPMP2MI_RETIME_OK || rest.status != GPMP2MI_RETIME_OK) return 31;
    if (!(cm.time_scale > 2.5) || !(cr.duration < 0.8 * cm.time_scale * 2.0) || !(cr.duration > lr.duration)) return 32;
    if (!(cr.achieved[0] <= 1.0 + 1e-9) || !(cr.achieved[1] <= 1.0 + 1e-9) || !(cr.achieved[3] <= 1.0 + 1e-9)) return 33;
    if (!(slow.duration >= 2.0 * (1.0 - 1e-12)) || !(slow.duration >= cr.duration)) return 34;
    if (rest.sdot[0] != 0.0 || rest.sdot[Md - 1] != 0.0 || !(rest.duration >= cr.duration) || !std::isfinite(rest.duration)) return 35;
    for (std::size_t k = 0; k + 1 < Md; k++)
      if (!(cr.stamps[k + 1] > cr.stamps[k]) || !(slow.sdot[k] <= 1.0)) return 36;
    const RetimedTrajectory over = RetimeTrajectory(model, limits, corner, setting, J, 2.0, 2.5);
    if (over.status != GPMP2MI_RETIME_BOUNDARY || over.duration != inf || over.sdot[0] == over.sdot[0]) return 37;
    // the corner result is the cheaper one, and with a bound between the two durations it is not chosen
    const std::vector<TrajectoryScore> clear{score(0.5, 0), score(0.5, 0)};
    const int best = SelectBestTrajectory({2.0, 1.0}, {}, clear, {lm, cm}, {lr, cr}, -inf, 0.5 * (lr.duration + cr.duration), 0.0,
                                          false, &n);
    if (best != 0 || n != 1) return 38;
    std::printf("OK best=%d of %zu eligible\n", best, n);
    return 0;
  } catch (const std::exception& e) {
    std::printf("EXCEPTION %s\n", e.what());
    return 3;
  }
}
