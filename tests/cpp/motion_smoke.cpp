// Builds against include/gpmp2mi_planner.hpp with plain g++ and links the product library.  The selection overload that
// takes the motion scores is host code and runs everywhere; the scores need the GPU: without one they must throw (no
// silent fallback), with one a 3-link arm swung fast through its joint range is told from the same arm moved gently.
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

int main() {
  try {
    // the rule alone: row 1 is the cheapest but leaves its joint range, row 2 has a non-finite quantity, row 3 is too fast
    const double inf = std::numeric_limits<double>::infinity();
    const Vector fe{5.0, 1.0, 2.0, 3.0, 4.0, 0.5};
    const std::vector<int> status{0, 0, 0, 0, 1, GPMP2MI_TRAJ_NOT_SPD};
    const std::vector<TrajectoryScore> sc{score(0.1, 0), score(0.1, 0), score(0.1, 0), score(0.05, 0), score(0.2, 3), score(0.3, 0)};
    const std::vector<TrajectoryMotionScore> ms{motion(0.3, 0.9, 0), motion(-0.02, 0.5, 0), motion(0.5, 0.5, 2), motion(0.2, 1.7, 0),
                                                motion(0.01, 1.0, 0), motion(0.3, 0.2, 0)};
    std::size_t n = 99;
    if (SelectBestTrajectory(fe, status, sc, 0.0, false, &n) != 1 || n != 5) return 10;             // without the motion scores
    if (SelectBestTrajectory(fe, status, sc, ms, 0.0, 1.0, 0.0, false, &n) != 4 || n != 2) return 11;
    if (SelectBestTrajectory(fe, status, sc, ms, 0.0, 1.0, 0.0, true, &n) != 0 || n != 1) return 12;
    if (SelectBestTrajectory(fe, status, sc, ms, 0.0, 2.0, 0.0, false, &n) != 3 || n != 3) return 13;
    if (SelectBestTrajectory(fe, status, sc, ms, -inf, inf, 0.0, false, &n) != 1 || n != 4) return 14;   // invalid stays out
    if (SelectBestTrajectory(fe, status, sc, ms, 0.4, inf, 0.0, false, &n) != -1 || n != 0) return 15;
    bool threw = false;
    try {
      SelectBestTrajectory(fe, status, sc, ms, std::nan(""), 1.0);
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
    limits.pos_down = {-1.0, -2.0, -inf};
    limits.pos_up = {1.0, 2.0, inf};
    limits.vel = {1.0, 1.0, 1.0};
    limits.acc = {4.0, 4.0, 4.0};
    limits.point_speed = 1.0;
    TrajOptimizerSetting setting(3);
    setting.set_total_step(8);
    setting.set_total_time(2.0);
    // constant-velocity lines: 1.4 rad over 2 s in joint 0 ends outside its range; the gentle one stays inside everything
    const Trajectory fast = initArmTrajStraightLine({-0.2, 0.1, -0.1}, {1.2, 0.1, -0.1}, 8);
    const Trajectory gentle = initArmTrajStraightLine({0.2, 0.1, -0.1}, {0.5, -0.2, 0.3}, 8);
    Trajectory fast_v = fast, gentle_v = gentle;
    for (std::size_t i = 0; i <= 8; i++)
      for (std::size_t d = 0; d < 3; d++) {
        fast_v.data[i * 6 + 3 + d] = (fast.data[8 * 6 + d] - fast.data[d]) / 2.0;
        gentle_v.data[i * 6 + 3 + d] = (gentle.data[8 * 6 + d] - gentle.data[d]) / 2.0;
      }
    const TrajectoryMotionScore f = MotionScoreTrajectory(model, limits, fast_v, setting, 4);
    const TrajectoryMotionScore g = MotionScoreTrajectory(model, limits, gentle_v, setting, 4);
    std::printf("FAST margin=%.4f at (%d, %d) vel=%.4f acc=%.3g speed=%.4f at (%d, %d) scale=%.4f\nGENTLE margin=%.4f scale=%.4f\n",
                f.pos_margin, f.pos_state, f.pos_coord, f.vel_ratio, f.acc_ratio, f.point_speed, f.speed_state, f.speed_sphere,
                f.time_scale, g.pos_margin, g.time_scale);
    if (std::fabs(f.pos_margin + 0.2) > 1e-12 || f.pos_state != 40 || f.pos_coord != 0 || f.invalid != 0) return 22;
    if (std::fabs(f.vel_ratio - 0.7) > 1e-12 || f.vel_coord != 0 || !(f.acc_ratio < 1e-9)) return 23;
    // joint 0 alone moves: the outermost sphere (x = 1.375 of the stretched arm) is the fastest, 0.7 rad/s times its radius
    if (f.speed_sphere != 5 || !(f.point_speed > 0.7 * 1.2) || !(f.point_speed < 0.7 * 1.4) ||
        std::fabs(f.time_scale - f.point_speed) > 1e-12)
      return 24;
    if (!(g.pos_margin > 0.4) || !(g.time_scale < 1.0) || g.invalid != 0) return 25;
    const TrajectoryMotionScore none = MotionScoreTrajectory(model, MotionLimits{}, fast_v, setting, 4);
    if (none.pos_margin != inf || none.vel_ratio != 0.0 || none.acc_ratio != 0.0 || none.time_scale != 0.0 || none.pos_state != -1 ||
        none.point_speed != f.point_speed)
      return 26;
    // the fast result is the cheaper one, and is not chosen
    const std::vector<TrajectoryScore> clear{score(0.5, 0), score(0.5, 0)};
    const int best = SelectBestTrajectory({1.0, 2.0}, {}, clear, {f, g}, 0.0, 1.0, 0.0, false, &n);
    if (best != 1 || n != 1) return 27;
    std::printf("OK best=%d of %zu eligible\n", best, n);
    return 0;
  } catch (const std::exception& e) {
    std::printf("EXCEPTION %s\n", e.what());
    return 3;
  }
}
