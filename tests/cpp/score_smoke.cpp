// Builds against include/gpmp2mi_planner.hpp with plain g++ and links the product library.  The selection rule is
// host code and runs everywhere; scoring needs the GPU: without one it must throw (no silent fallback), with one it
// plans three restarts of a 2-link problem, scores them densely and picks one.
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

int main() {
  try {
    // the rule alone: row 1 is the cheapest but NOT_SPD, row 2 collides, rows 3 and 4 tie and 3 is the lower one
    const double inf = std::numeric_limits<double>::infinity();
    const Vector fe{5.0, 1.0, 2.0, 3.0, 3.0, std::nan("")};
    const std::vector<int> status{0, GPMP2MI_TRAJ_NOT_SPD, 0, 0, 1, 0};
    const std::vector<TrajectoryScore> sc{score(0.1, 0), score(0.1, 0), score(-0.02, 0), score(0.05, 3), score(0.2, 0), score(0.3, 0)};
    std::size_t n = 99;
    if (SelectBestTrajectory(fe, status, sc, 0.0, false, &n) != 3 || n != 3) return 10;
    if (SelectBestTrajectory(fe, status, sc, 0.0, true, &n) != 4 || n != 2) return 11;
    if (SelectBestTrajectory(fe, status, sc, -inf, false, &n) != 2 || n != 4) return 12;
    if (SelectBestTrajectory(fe, {}, sc, -inf) != 1) return 13;
    if (SelectBestTrajectory(fe, status, sc, 1.0, false, &n) != -1 || n != 0) return 14;
    std::printf("SELECT OK\n");

    Arm arm(2, {1.0, 1.0}, {0.0, 0.0}, {0.0, 0.0}, Pose3::Translation(0.0, 0.0, 0.0));
    BodySphereVector spheres;
    for (int l = 0; l < 2; l++)
      for (double x : {-0.75, -0.25}) spheres.emplace_back(l, 0.1, std::array<double, 3>{x, 0.0, 0.0});
    ArmModel model(arm, spheres);
    const int cells = 60;
    Vector field(cells * cells);  // distance to a disc of radius 0.4 at (1.2, 1.0); column-major (row = y, col = x)
    for (int x = 0; x < cells; x++)
      for (int y = 0; y < cells; y++)
        field[x * cells + y] = std::hypot(-3.0 + 0.1 * x - 1.2, -3.0 + 0.1 * y - 1.0) - 0.4;
    PlanarSDF sdf({-3.0, -3.0}, 0.1, cells, cells, field);
    TrajOptimizerSetting setting(2);
    setting.set_total_step(10);
    setting.set_total_time(2.0);
    setting.set_obs_check_inter(2);
    setting.set_cost_sigma(0.1);
    setting.set_epsilon(0.2);
    setting.setGaussNewton();
    const Vector start{0.0, 0.0}, end{1.5, 0.5}, zero{0.0, 0.0};
    Vector errs;
    std::vector<TrajectoryScore> scores;
    for (double bump : {0.0, 0.6, -0.6}) {
      Trajectory init = initArmTrajStraightLine(start, end, 10);
      for (std::size_t i = 0; i <= 10; i++) init.x(i)[0] += bump * std::sin(M_PI * static_cast<double>(i) / 10.0);
      int iters = 0;
      double err = 0;
      const Trajectory out = BatchTrajOptimize2DArm(model, sdf, start, zero, end, zero, init, setting, &iters, &err);
      const TrajectoryScore s0 = ScoreTrajectory(model, sdf, out, setting, 0), s4 = ScoreTrajectory(model, sdf, out, setting, 4);
      // inter_step = 0 is CollisionCost2DArm; more checked states can only add cost and lower the clearance
      const double cc = CollisionCost2DArm(model, sdf, out, setting);
      if (std::fabs(s0.support_cost - cc) > 1e-12 + 1e-8 * std::fabs(cc) || s0.dense_cost != s0.support_cost) return 20;
      if (s4.support_cost != s0.support_cost || s4.dense_cost < s4.support_cost || s4.min_clearance > s0.min_clearance) return 21;
      if (s4.worst_state < 0 || s4.worst_state > 50 || s4.worst_sphere < 0 || s4.worst_sphere > 3 || s4.out_of_range != 0) return 22;
      std::printf("RESTART bump=%.1f iterations=%d final_error=%.6f support=%.4f dense=%.4f clearance=%.4f at (%d, %d)\n", bump,
                  iters, err, s4.support_cost, s4.dense_cost, s4.min_clearance, s4.worst_state, s4.worst_sphere);
      errs.push_back(err);
      scores.push_back(s4);
    }
    const int best = SelectBestTrajectory(errs, {}, scores, -inf, true, &n);
    if (best < 0 || n != 3) return 23;
    for (double e : errs)
      if (e < errs[best]) return 24;
    std::printf("OK best=%d of %zu eligible\n", best, n);
    return 0;
  } catch (const std::exception& e) {
    std::printf("EXCEPTION %s\n", e.what());
    return 3;
  }
}
